"""The device sensor and truth on a batch of multi-hypothesis FastSLAM filters (include/rfsgpu.h [sensor]:
rfsgpu_batch_fastslam_serve_sensor, rfsgpu_batch_fastslam_mh_cycle_sensed_async; csrc/fastslam_sensed.h): the sensed cycle against the
host-fed cycle on a twin that is handed the first handle's scans and the restated resampling draws, the run call against the per-step
calls, and the simulator loop -- bit for bit: the sensed route runs the host-fed route's kernels on records whose derived fields (pfa,
prune, the count, the draw) must have the host's bits."""
import ctypes as C

import numpy as np
import pytest

from tests.support import device_loop_reference as dl
from tests.support import sensor_reference as sr

NF, N0, STRIDE, STEPS, QUIET = 4, 5, 65, 14, 4      # (65 >= nParticlesMax 15 x 4 hypotheses, and no multiple of 64)
HYPS = [3, 1, 4, 3]
PRUNE_AT = [0, 4, 0, 4]
DENSE = 12.0 / (2 * np.pi * 2.0)                    # clutter intensity whose mean over [0.5, 2.5] is 12
R_SENSOR = np.diag([5e-4, 5e-5])
MOTION_SEED = 500


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


def _scens(sc):
    return [sc.make_scenario(N0, 12, 8, seed=112 + b) for b in range(NF)]


def _sensors(scens):
    """Filter 0 never sees anything (Pd 0, no clutter); filter 1 stands far from its landmarks for the first QUIET steps; filter 2 has
    dense clutter over six landmarks; filter 3 sees six landmarks with Pd 0.6, so that its counts lie on both sides of its
    pruningMeasurementsThreshold 4."""
    out = []
    for b, s in enumerate(scens):
        out.append(dict(R=R_SENSOR, Pd=[0.0, 0.9, 0.4, 0.6][b], clutter=[0.0, 0.0, DENSE, 1e-4][b], rmax=2.5, rmin=0.5,
                        lm=s["gt"][: [12, 12, 6, 6][b]], seed=9100 + b))
    return out


def _inputs(nF=NF, steps=STEPS):
    rng = np.random.default_rng(4)
    gt = np.zeros((steps + 1, nF, 3))
    u = np.zeros((steps + 1, nF, 3))
    for k in range(1, steps + 1):
        u[k] = rng.uniform(-1, 1, (nF, 3)) * [0.01, 0.004, 0.01]
        gt[k] = gt[k - 1] + u[k]
    gt[1:QUIET + 1, 1, :2] += 50.0
    return gt, u


def _batch(pkg, scens, stride=STRIDE, hyps=HYPS):
    nF = len(scens)
    B = pkg.MHFastSLAMBatch(nF, N0, stride, gm_capacity=512, metrics=True)
    x = np.zeros((nF * stride, 3))
    for b, s in enumerate(scens):
        P = s["params"]
        B.configure(b, None, R=P["R"], Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"], kf=(P["kf_range"], P["kf_bearing"]),
                    Q=P["Q_lm"])
        x[b * stride:b * stride + N0] = s["poses"]
        for i in range(N0):
            B.import_gm(b * stride + i, np.zeros(s["w"][i].shape), s["mean"][i], s["cov"][i])
        c = B.default_fastslam_config()
        c.maxNDataAssocHypotheses = hyps[b]
        c.maxDataAssocLogLikelihoodDiff = 50.0
        c.nParticlesMax = 3 * N0
        c.minUpdatesBeforeResample = 1
        c.minMeasurementsBeforeResample = 1
        c.pruningMeasurementsThreshold = PRUNE_AT[b]
        if b == 2:      # the dense clutter's landmarks go at the next prune: the association table stays within Murty's 64
            c.mapExistencePruneThreshold = 0.2
        B.configure_fastslam(b, c)
        B.set_motion_odometry(b, [2e-5, 2e-5, 1e-5], MOTION_SEED + b)
        B.set_resampling(b, 4.0, 0.8)
        B.set_ground_truth(s["gt"], np.zeros(len(s["gt"])), filter=b)
    B.set_poses(x, scens[0]["pose_cov"])
    B.set_weights(np.ones(nF * stride))
    return B


def _set_sensors(B, sensors, max_nz=64):
    for b, s in enumerate(sensors):
        B.set_sensor(b, s["R"], s["Pd"], s["clutter"], s["rmax"], s["rmin"], s["lm"], max_nz=max_nz, seed=s["seed"])


def _live_state(B, only=None):
    """Everything the C ABI shows of the live slots, as tests/test_mh_fastslam_batch.py compares it (Rig.block_state and the ids)."""
    counts = B.live_counts()
    w, x, sizes, masks = B.get_weights(), B.get_poses(), np.asarray(B.gm_sizes()), np.asarray(B.get_unused_masks())
    ids, pids = B.get_particle_ids()
    out = dict(counts=counts.copy() if only is None else counts[list(only)].copy())
    for b in (range(B.n_filters) if only is None else only):
        blk = B.block(b, counts[b])
        out[b] = dict(w=_bits(w[blk]), poses=_bits(x[blk]), sizes=sizes[blk].copy(), masks=masks[blk].copy(), ids=np.asarray(ids)[blk].copy(),
                      pids=np.asarray(pids)[blk].copy(), fov=np.array([B.landmarks_in_fov(i) for i in range(blk.start, blk.stop)]),
                      gm=[[_bits(a) for a in B.export_gm(i)] for i in range(blk.start, blk.stop)])
    return out


def _assert_same(sa, sb, what):
    assert sa.keys() == sb.keys(), what
    np.testing.assert_array_equal(sa["counts"], sb["counts"], err_msg=f"{what}: live counts")
    for b in sa:
        if b == "counts":
            continue
        for key in ("w", "poses", "sizes", "masks", "ids", "pids", "fov"):
            np.testing.assert_array_equal(sa[b][key], sb[b][key], err_msg=f"{what}: filter {b}: {key}")
        for i, (ga, gb) in enumerate(zip(sa[b]["gm"], sb[b]["gm"])):
            for p, q in zip(ga, gb):
                np.testing.assert_array_equal(p, q, err_msg=f"{what}: filter {b}: mixture of live slot {i}")


def _assert_same_last_cycle(la, lb, what):
    assert la.keys() == lb.keys()
    for key in la:
        a, b = (np.asarray(v) for v in (la[key], lb[key]))
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b, err_msg=f"{what}: last_cycle {key}")


def _restated_counts(scens, sensors, gt, steps):
    from test_batch_sensed_cycle import _assert_clear_of_the_limits
    restated = [[sr.scan(gt[k, b], s["lm"], s["R"], s["Pd"], s["clutter"], s["rmin"], s["rmax"], s["seed"], k) for b, s in enumerate(sensors)]
                for k in range(1, steps + 1)]
    for k, row in enumerate(restated):
        for (_, info), s in zip(row, sensors):
            _assert_clear_of_the_limits(info, s["rmin"], s["rmax"], (k + 1, s["seed"]))
    return np.array([[len(Z) for Z, _ in row] for row in restated])


def test_the_premises_on_the_restated_counts(pkg, sc):
    """What the GPU tests below rest on, checked with the restatement alone (no GPU): an idle filter, one that goes from empty to
    non-empty scans, counts on both sides of a pruningMeasurementsThreshold WITH measurements, and a dense-clutter filter whose
    association table (12 landmarks at most from the start, the last scan's new ones, this scan) stays within Murty's 64."""
    scens = _scens(sc)
    gt, _ = _inputs()
    counts = _restated_counts(scens, _sensors(scens), gt, STEPS)
    assert counts[:, 0].max() == 0
    assert counts[:QUIET, 1].max() == 0 and counts[QUIET, 1] > 0
    assert counts[:, 2].min() >= 6
    assert ((counts[:, 3] > 0) & (counts[:, 3] < PRUNE_AT[3])).any() and (counts[:, 3] >= PRUNE_AT[3]).any()
    assert (12 + counts[:-1, 2] + counts[1:, 2]).max() <= 64 and 12 + counts[0, 2] <= 64


@pytest.mark.gpu
def test_sensed_cycle_equals_the_host_fed_cycle_on_the_same_scans(pkg, sc):
    scens = _scens(sc)
    sensors = _sensors(scens)
    gt, u = _inputs()
    counts = _restated_counts(scens, sensors, gt, STEPS)
    A, B = _batch(pkg, scens), _batch(pkg, scens)
    A.serve_sensor(True)
    _set_sensors(A, sensors)
    for bt in (A, B):
        bt.error_log_create(STEPS)
    grew = shrank = idle_seen = False
    prev = np.full(NF, N0)
    for k in range(1, STEPS + 1):
        t = np.full(NF, 0.1 * k)
        A.propagate_async(u[k], k)
        A.sense_async(gt[k], k)
        Zs = A.last_scan()
        nz = np.array([len(Z) for Z in Zs])
        np.testing.assert_array_equal(nz, counts[k - 1], err_msg=f"step {k}: counts against the restatement")
        A.fastslam_mh_cycle_sensed_async(True, k)
        A.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        B.propagate_async(u[k], k)
        B.cycle_async(True, Zs, [dl.resample_draw(MOTION_SEED + b, k) for b in range(NF)])
        B.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        la, lb = A.last_cycle(), B.last_cycle()
        _assert_same_last_cycle(la, lb, f"step {k}")
        _assert_same(_live_state(A), _live_state(B), f"step {k}")
        grew |= bool((la["n_after_update"] > prev).any())
        shrank |= bool((la["fired"] & (la["n_after_resample"] < la["n_after_update"])).any())
        # a filter with an empty scan only counted the update: identity parents and plans, nothing fired, no N_eff -- on BOTH handles,
        # of which the sensed one knows the count from the device's records alone
        for b in np.nonzero(nz == 0)[0]:
            n = int(prev[b])
            assert la["n_after_update"][b] == la["n_after_resample"][b] == n and not la["fired"][b] and la["n_eff"][b] == 0.0
            np.testing.assert_array_equal(la["parent"][b, :n], np.arange(n))
            idle_seen = True
        prev = la["n_after_resample"].copy()
    assert grew and shrank and idle_seen
    ea, eb = A.error_log_read(), B.error_log_read()
    assert ea.shape[0] == STEPS and ea.tobytes() == eb.tobytes()
    A.close()
    B.close()


@pytest.mark.gpu
def test_capacity_stays_per_filter(pkg, sc):
    """A stride that filter 2's growth (4 hypotheses) exceeds: the sensed handle reports RFSGPU_ERR_CAPACITY naming the filter the
    host-fed twin names, and the other filters' bits match."""
    scens = _scens(sc)
    sensors = _sensors(scens)
    gt, u = _inputs()
    stride = 16
    A, B = _batch(pkg, scens, stride=stride), _batch(pkg, scens, stride=stride)
    A.serve_sensor(True)
    _set_sensors(A, sensors)
    named = []
    for k in range(1, 4):
        A.propagate_async(u[k], k)
        A.sense_async(gt[k], k)
        Zs = A.last_scan()
        A.fastslam_mh_cycle_sensed_async(True, k)
        B.propagate_async(u[k], k)
        B.cycle_async(True, Zs, [dl.resample_draw(MOTION_SEED + b, k) for b in range(NF)])
        errs = []
        for bt in (A, B):
            try:
                bt.synchronize()
                errs.append(None)
            except pkg.capi.EngineError as e:
                assert e.status == pkg.capi.ERR_CAPACITY, str(e)
                errs.append(str(e)[str(e).index("filter "):].split(":")[0])
        assert errs[0] == errs[1], (k, errs)
        named += [e for e in errs[:1] if e]
        la, lb = A.last_cycle(), B.last_cycle()
        np.testing.assert_array_equal(la["overflowed"], lb["overflowed"])
        ok = [b for b in range(NF) if not la["overflowed"][b]]
        _assert_same(_live_state(A, ok), _live_state(B, ok), f"step {k}")
    assert named, "no filter outgrew the stride: the test does not reach the overflow"
    A.close()
    B.close()


RUN_K = 40


def _run_setup(pkg, seeds=(11, 12, 13), sensor=True, log=True, motion=True):
    """3 filters of 8 particles, stride 72, with different Pd and clutter; truth of RUN_K steps of which the first 10 are pinned."""
    sim = pkg.sim2d_driver
    base = dict(sim.C1_FASTSLAM_SIM, kmax=RUN_K, n_landmarks=10, eff_n=6.0, max_hypotheses=3)
    Ps = [dict(base, Pd=0.99, clutter=1e-4), dict(base, Pd=0.7, clutter=5e-3, eff_n=4.0), dict(base, Pd=0.9, clutter=1e-3)]
    batch = pkg.MHFastSLAMBatch(3, 8, 72, gm_capacity=256, metrics=True)
    for b, P in enumerate(Ps):
        c = sim.configure_fastslam_batch_filter(batch, b, P)
        c.nParticlesMax = 24
        batch.configure_fastslam(b, c)
        Q = np.array([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2
        if motion or b != 1:
            batch.set_motion_odometry(b, Q, seeds[b])
        batch.set_resampling(b, P["eff_n"], 0.75)
        t = sim.truth_config(P, b)
        t.n_still, t.n_pinned = 2, 10
        batch.set_truth(b, t, seeds[b])
    batch.serve_sensor(True)
    batch.generate_truth(RUN_K)
    truth = [batch.get_truth(b) for b in range(3)]
    for b, (P, d) in enumerate(zip(Ps, truth)):
        if sensor or b != 2:
            batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                             max_nz=sim.sensor_max_nz_of(d["n_det_max"], P), seed=seeds[b])
        batch.set_ground_truth(d["landmarks"], d["first_seen"], filter=b)
    if log:
        batch.error_log_create(RUN_K)
    return batch, Ps, truth


@pytest.mark.gpu
def test_the_run_call_equals_the_per_step_calls(pkg):
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    A, Ps, _ = _run_setup(pkg)
    A.run_truth_async(1, RUN_K, True, *consts)
    sA, logA, scanA, lcA = _live_state(A), A.error_log_read(), A.last_scan(), A.last_cycle()
    assert logA.shape == (RUN_K - 1, 3) and max(s.max() for b, v in sA.items() if b != "counts" for s in [v["sizes"]]) > 0
    B, _, truthB = _run_setup(pkg)
    gt = np.ascontiguousarray(np.stack([d["gt"] for d in truthB], axis=1))
    od = np.ascontiguousarray(np.stack([d["odom"] for d in truthB], axis=1))
    pin = np.ones(3, dtype=np.uint8)
    for k in range(1, RUN_K):
        if k <= 10:
            B.propagate_async(od[k], k, pin=pin, pin_pose=gt[k])
        else:
            B.propagate_async(od[k], k)
        B.sense_async(gt[k], k)
        B.fastslam_mh_cycle_sensed_async(True, k)
        B.step_error_async(np.array([k * P["dt"] for P in Ps]), gt[k], *consts)
    _assert_same(sA, _live_state(B), "run call against per-step calls")
    _assert_same_last_cycle(lcA, B.last_cycle(), "run call against per-step calls")
    assert logA.tobytes() == B.error_log_read().tobytes()
    for za, zb in zip(scanA, B.last_scan()):
        np.testing.assert_array_equal(_bits(za), _bits(zb))
    Cc, _, _ = _run_setup(pkg)
    Cc.run_truth_async(1, 17, True, *consts)
    Cc.run_truth_async(17, RUN_K, True, *consts)
    _assert_same(sA, _live_state(Cc), "two calls against one")
    assert Cc.error_log_read().tobytes() == logA.tobytes()
    D, _, _ = _run_setup(pkg, log=False)
    D.run_truth_async(1, 17)
    D.run_truth_async(17, RUN_K)
    _assert_same(sA, _live_state(D), "without the error log")
    I = pkg.capi.ERR_INVALID
    for kw, args, needles in ((dict(sensor=False), (1, RUN_K), ("filter 2", "rfsgpu_batch_set_sensor")),
                              (dict(motion=False), (1, RUN_K), ("filter 1", "rfsgpu_batch_set_motion_odometry")),
                              (dict(log=False), (1, RUN_K, True) + consts, ("rfsgpu_error_log_create",))):
        E, _, _ = _run_setup(pkg, **kw)
        s0 = _live_state(E)
        _raises(pkg, I, lambda: E.run_truth_async(*args), "batch_run_truth", *needles)
        _assert_same(s0, _live_state(E), str(kw))
        E.close()
    for bt in (A, B, Cc, D):
        bt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_truth", [False, True])
def test_the_simulator_loop_with_the_device_sensor(pkg, device_truth):
    from test_batch_sensed_cycle import _assert_clear_of_the_limits
    sim = pkg.sim2d_driver
    nF, n, K = 3, 8, 40
    Ps = [dict(sim.C1_FASTSLAM_SIM, kmax=K, n_landmarks=10, Pd=pd, clutter=c, max_hypotheses=3, eff_n=6.0) for pd, c in ((0.99, 1e-4), (0.7, 5e-3), (0.9, 1e-3))]
    datas = None if device_truth else [sim.generate(P, traj_seed=1 + b, kmax=K, measurements=False) for b, P in enumerate(Ps)]
    seeds = [100 + b for b in range(nF)]
    logs, states = [], []
    for _ in range(2):
        batch = pkg.MHFastSLAMBatch(nF, n, 72, gm_capacity=256)
        if device_truth:
            run = sim.Sim2dMHBatchRun(batch, None, Ps, seeds, track_errors=True, device_truth=True, kmax=K)
        else:
            run = sim.Sim2dMHBatchRun(batch, datas, Ps, seeds, track_errors=True, device_sensor=True)
        assert run.device_loop and not hasattr(run, "_z") and not hasattr(run, "_nz") and not hasattr(run, "u01")
        run.run(1, K)
        scans = batch.last_scan()
        for b, P in enumerate(Ps):
            d = batch.get_truth(b) if device_truth else datas[b]
            want, info = sr.scan(d["gt"][K - 1], d["landmarks"], np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmin"], P["rmax"], seeds[b], K - 1)
            _assert_clear_of_the_limits(info, P["rmin"], P["rmax"], b)
            assert not info["cut"] and scans[b].shape == want.shape
            np.testing.assert_allclose(scans[b], want, rtol=1e-10, atol=1e-10)
        log = run.errors()
        assert log.shape == (K - 1, nF) and np.isfinite(log["cola"]).all() and np.isfinite(log["pose_ed"]).all()
        logs.append(log.tobytes())
        states.append(_live_state(batch))
        batch.close()
    assert logs[0] == logs[1]
    _assert_same(states[0], states[1], "two runs")


@pytest.mark.gpu
def test_refusals_and_call_order(pkg, sc):
    U, I = pkg.capi.ERR_UNSUPPORTED, pkg.capi.ERR_INVALID
    scens = _scens(sc)
    sensors = _sensors(scens)
    gt, u = _inputs()
    A = _batch(pkg, scens)
    s0 = _live_state(A)
    # before the switch: as always
    _raises(pkg, U, lambda: A.sense_async(gt[1], 1), "multi-hypothesis", "rfsgpu_batch_fastslam_serve_sensor")
    _raises(pkg, U, lambda: A.fastslam_mh_cycle_sensed_async(True, 1), "multi-hypothesis")
    A.serve_sensor(True)
    _set_sensors(A, sensors)
    # a sensed cycle without a fresh sense call; the other kinds' calls name the right one
    _raises(pkg, I, lambda: A.fastslam_mh_cycle_sensed_async(True, 1), "rfsgpu_batch_sense_async")
    A.sense_async(gt[1], 1)
    _raises(pkg, U, lambda: A.cycle_sensed_async(True), "rfsgpu_batch_fastslam_mh_cycle_sensed_async")
    _raises(pkg, U, lambda: A.fastslam_cycle_sensed_async(True), "rfsgpu_batch_fastslam_mh_cycle_sensed_async")
    _raises(pkg, U, lambda: A.resample_sensed_async(1), "multi-hypothesis", "resamples inside the cycle")
    _assert_same(s0, _live_state(A), "after the refusals")
    # the multi-hypothesis call on the other kinds
    fs = pkg.FastSLAMBatch(2, 4, gm_capacity=16)
    fs.configure_fastslam(None, pkg.sim2d_driver.fastslam_config(fs))
    fs.serve_sensor(True)
    rb = pkg.FilterBatch(2, 4, gm_capacity=16)
    rb.cycle_async(True, [np.zeros((0, 2))] * 2, normalize=True)      # (empty scans: the call alone decides the kind)
    for f, needle in ((fs, "rfsgpu_batch_fastslam_cycle_sensed_async"), (rb, "rfsgpu_batch_cycle_sensed_async")):
        w0 = f.get_weights().copy()
        _raises(pkg, U, lambda: f._call("batch_fastslam_mh_cycle_sensed_async", C.c_int(1), C.c_void_p(None), C.c_void_p(None), C.c_int(0), C.c_ulonglong(1)), needle)
        np.testing.assert_array_equal(f.get_weights(), w0)
    _raises(pkg, U, lambda: rb.fastslam_cycle_sensed_async(True), "rfsgpu_batch_cycle_sensed_async")
    # a filter without a motion key has no draw
    nokey = pkg.MHFastSLAMBatch(2, 4, 16, gm_capacity=16)
    nokey.set_motion_odometry(0, [1e-4, 1e-4, 1e-4], 1)
    nokey.serve_sensor(True)
    nokey.set_sensor(None, R_SENSOR, 0.9, 0.0, 2.5, 0.5, np.array([[1.0, 0.0]]), seed=3)
    nokey.sense_async(np.zeros((2, 3)), 1)
    _raises(pkg, I, lambda: nokey.fastslam_mh_cycle_sensed_async(True, 1), "filter 1", "rfsgpu_batch_set_motion_odometry")
    # after a sensed cycle: the host-fed cycle refuses, and the switch stays on
    A.fastslam_mh_cycle_sensed_async(True, 1)
    A.synchronize()
    s1 = _live_state(A)
    Zs = A.last_scan()
    _raises(pkg, U, lambda: A.cycle_async(True, Zs, [0.5] * NF), "sensed cycle")
    _raises(pkg, I, lambda: A.serve_sensor(False), "sensed cycle")
    _assert_same(s1, _live_state(A), "after the refusals behind a sensed cycle")
    for f in (A, fs, rb, nokey):
        f.close()
