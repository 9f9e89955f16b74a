"""The device sensor and truth on a batch of FastSLAM filters (include/rfsgpu.h [sensor]: rfsgpu_batch_fastslam_serve_sensor,
rfsgpu_batch_fastslam_cycle_sensed_async; csrc/fastslam_sensed.h): the sensed cycle against the host-fed cycle on a twin that is handed
the first handle's scans, the run call against the per-step calls, and the simulator loop -- all bit for bit, because the sensed route
runs the host-fed route's kernels on records whose three derived fields (pfa, prune, the count) must have the host's bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import sensor_reference as sr

NEW_SYMBOLS = {"rfsgpu_batch_fastslam_serve_sensor": 2, "rfsgpu_batch_fastslam_cycle_sensed_async": 6,
               "rfsgpu_batch_fastslam_mh_cycle_sensed_async": 6}     # name -> C arguments

NF, NP, STEPS, QUIET = 5, 65, 12, 4       # (65: one past a wavefront, so the filters' blocks straddle waves)
DENSE = 12.0 / (2 * np.pi * 2.0)          # clutter intensity whose mean over [0.5, 2.5] is 12
R_SENSOR = np.diag([5e-4, 5e-5])
SMALL_BOUND = 48                          # the second max_nz bound (no restated scan reaches it)
PRUNE_AT = [0, 4, 0, 3, 5]                # pruningMeasurementsThreshold per filter


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_agree_on_the_new_calls(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfsgpu.h")).read(), flags=re.S)
    pkg.build_mod.build()
    lib = pkg.load_library()
    src = open(os.path.join(ROOT, "rfs-slam_amd", "capi.py")).read()
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name + " is not declared in rfsgpu.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name + " is not exported"
        short = name[len("rfsgpu_"):]
        assert short in pkg.capi.ABI_SYMBOLS
        # every binding call passes the handle (added by _call) + nargs - 1 arguments
        calls = re.findall(r'self\._call\("' + short + r'",(.*?)\)\n', src, flags=re.S)
        assert calls, short + " is not bound in capi.py"
        for c in calls:
            depth, n = 0, 1
            for ch in c:
                depth += ch in "(["
                depth -= ch in ")]"
                n += (ch == "," and depth == 0)
            assert n == nargs - 1, (short, n)
    raw = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()      # (with its comments: the section headings live there)
    for name in NEW_SYMBOLS:
        assert raw.index("/* ---- [sensor]") < raw.index("int " + name + "(") < raw.index("/* ---- [truth]"), name + " is not in the [sensor] section"
    for meth in ("serve_sensor", "fastslam_cycle_sensed_async"):
        assert hasattr(pkg.capi.CBatch, meth)
    assert hasattr(pkg.capi.CBatchMH, "fastslam_mh_cycle_sensed_async")
    # a null handle is refused before anything else
    null = C.c_void_p()
    for name in NEW_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    assert lib.rfsgpu_batch_fastslam_serve_sensor(null, C.c_int(1)) == pkg.capi.ERR_INVALID
    assert lib.rfsgpu_batch_fastslam_cycle_sensed_async(null, C.c_int(1), null, null, C.c_int(0), C.c_int(1)) == pkg.capi.ERR_INVALID
    assert lib.rfsgpu_batch_fastslam_mh_cycle_sensed_async(null, C.c_int(1), null, null, C.c_int(0), C.c_ulonglong(1)) == pkg.capi.ERR_INVALID


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_switch_is_for_the_two_fastslam_kinds_only(pkg):
    """UNSUPPORTED, naming which, on an RB-PHD batch that has cycled, an ordinary handle, a group shard and a batch whose kind is open;
    before the switch every [sensor] call refuses a FastSLAM batch as it always has; off again: the refusals are back."""
    from test_batch_sensor import _section_calls
    U = pkg.capi.ERR_UNSUPPORTED
    rb = pkg.FilterBatch(2, 4, gm_capacity=16)
    rb.cycle_async(True, [np.zeros((0, 2))] * 2, normalize=True)      # (empty scans: the call alone decides the kind)
    single = pkg.RBPHDFilter(8, gm_capacity=16)
    group = pkg.FilterGroup(16, [0, 0], gm_capacity=16)
    open_kind = pkg.FilterBatch(2, 4, gm_capacity=16)
    for f, what in ((rb, "RB-PHD"), (single, "ordinary handle"), (group.shards[0], "shard"), (open_kind, "not decided")):
        w0 = f.get_weights().copy()
        for on in (1, 0):
            _raises(pkg, U, lambda: f._call("batch_fastslam_serve_sensor", C.c_int(on)), "batch_fastslam_serve_sensor", what)
        np.testing.assert_array_equal(f.get_weights(), w0)
    fs = pkg.FastSLAMBatch(2, 4, gm_capacity=16)
    fs.configure_fastslam(0, pkg.sim2d_driver.fastslam_config(fs))
    w0 = fs.get_weights().copy()
    for call in _section_calls(pkg.capi, fs, 2):
        _raises(pkg, U, call, "FastSLAM", "rfsgpu_batch_fastslam_serve_sensor")
    _raises(pkg, U, lambda: fs.fastslam_cycle_sensed_async(True), "FastSLAM")
    _raises(pkg, U, lambda: fs.run_truth_async(1, 2), "FastSLAM")
    fs.serve_sensor(True)
    fs.set_sensor(None, R_SENSOR, 0.9, 0.0, 2.5, 0.5, np.array([[1.0, 0.0]]), seed=3)
    fs.serve_sensor(False)
    for call in _section_calls(pkg.capi, fs, 2):
        _raises(pkg, U, call, "FastSLAM")
    np.testing.assert_array_equal(fs.get_weights(), w0)
    group.close()


def _batch(pkg, scens):
    """The scenarios of tests/test_batch_sensed_cycle.py as FastSLAM maps: the Gaussians' weights become log-odds."""
    from test_filter_batch import _configure_from_scenario
    batch = pkg.FastSLAMBatch(NF, NP, gm_capacity=512)
    batch.set_poses(np.vstack([s["poses"] for s in scens]), np.vstack([np.tile(np.asarray(s["pose_cov"], dtype=np.float64).ravel(), (NP, 1)) for s in scens]))
    batch.set_weights(np.concatenate([s["particle_w"] for s in scens]))
    for b, s in enumerate(scens):
        _configure_from_scenario(pkg.capi, batch, b, s["params"])
        c = batch.default_fastslam_config()
        c.pruningMeasurementsThreshold = PRUNE_AT[b]
        c.minUpdatesBeforeResample = 1
        c.minMeasurementsBeforeResample = 1
        batch.configure_fastslam(b, c)
        for i in range(NP):
            batch.import_gm(b * NP + i, np.log(s["w"][i] / (1 - s["w"][i] * 0.5)), s["mean"][i], s["cov"][i])
        batch.set_motion_odometry(b, [2e-5, 2e-5, 1e-5], 500 + b)
        batch.set_resampling(b, 0.98 * NP, 0.98)
    return batch


@pytest.mark.gpu
def test_sensed_cycle_equals_the_host_fed_cycle_on_the_same_scans(pkg, sc):
    from test_batch_sensed_cycle import _assert_clear_of_the_limits, _assert_same, _inputs, _sensors, _set_sensors, _state
    scens = [sc.make_scenario(NP, 40, 10, seed=901 + b) for b in range(NF)]
    sensors = _sensors(scens)
    gt, u = _inputs()
    # what the sensors will deliver, by the restatement: the premises of this test
    restated = [[sr.scan(gt[k, b], s["lm"], s["R"], s["Pd"], s["clutter"], s["rmin"], s["rmax"], s["seed"], k) for b, s in enumerate(sensors)]
                for k in range(1, STEPS + 1)]
    counts = np.array([[len(Z) for Z, _ in row] for row in restated])
    for k, row in enumerate(restated):
        for (_, info), s in zip(row, sensors):
            _assert_clear_of_the_limits(info, s["rmin"], s["rmax"], (k + 1, s["seed"]))
    assert counts[:, 0].max() == 0                                                    # one filter never sees anything
    assert counts[:QUIET, 1].max() == 0 and counts[QUIET, 1] > 0                      # one goes from empty scans to non-empty ones
    assert counts[:, 2].min() >= 12 and counts.max() < SMALL_BOUND                    # dense clutter; both bounds hold every scan
    thr = np.array(PRUNE_AT)
    crosses = [(counts[:, b] < thr[b]).any() and (counts[:, b] >= thr[b]).any() for b in range(NF)]
    assert any(crosses), "no filter is below its pruningMeasurementsThreshold in one step and at or above it in another"
    A, B, A_free, A_small = (_batch(pkg, scens) for _ in range(4))
    for bt in (A, A_free, A_small):
        bt.serve_sensor(True)
    _set_sensors(A, sensors, 64)
    _set_sensors(A_free, sensors, 64)
    _set_sensors(A_small, sensors, SMALL_BOUND)
    for bt in (A, B):
        for b, s in enumerate(scens):
            bt.set_ground_truth(s["gt"], np.zeros(len(s["gt"])), filter=b)
        bt.error_log_create(STEPS)
    fired_any = False
    went_nonempty = False
    last_nz = np.zeros(NF, dtype=int)
    for k in range(1, STEPS + 1):
        t = np.full(NF, 0.1 * k)
        A.propagate_async(u[k], k)
        A.sense_async(gt[k], k)
        Zs = A.last_scan()
        nz = np.array([len(Z) for Z in Zs])
        np.testing.assert_array_equal(nz, counts[k - 1], err_msg=f"step {k}: counts against the restatement")
        A.fastslam_cycle_sensed_async(True, normalize=True)
        A.resample_sensed_async(k)
        A.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        B.propagate_async(u[k], k)
        B.batch_fastslam_cycle_async(True, Zs, normalize=True)
        B.resample_async(nz, k)
        B.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        for bt in (A_free, A_small):
            bt.propagate_async(u[k], k)
            bt.sense_async(gt[k], k)
            bt.fastslam_cycle_sensed_async(True, normalize=True)
            bt.resample_sensed_async(k)
        _assert_same(_state(A), _state(B), f"step {k}")
        la, lb = A.last_resample(), B.last_resample()
        np.testing.assert_array_equal(la[0], lb[0], err_msg=f"step {k}: fired")
        np.testing.assert_array_equal(la[1], lb[1], err_msg=f"step {k}: plan")
        np.testing.assert_array_equal(_bits(la[2]), _bits(lb[2]), err_msg=f"step {k}: N_eff")
        fired_any |= bool(la[0].any())
        went_nonempty |= bool(((last_nz == 0) & (nz > 0) & (k > 1)).any())
        last_nz = nz
    assert fired_any, "no resampling fired"
    assert went_nonempty
    np.testing.assert_array_equal(A.resample_counts(), B.resample_counts())
    ea, eb = A.error_log_read(), B.error_log_read()
    assert ea.shape[0] == STEPS and ea.tobytes() == eb.tobytes()
    sa = _state(A)
    _assert_same(sa, _state(A_free), "the free-running handle")
    _assert_same(sa, _state(A_small), f"max_nz {SMALL_BOUND} against 64")
    for bt in (A_free, A_small):
        for x, y in zip(bt.last_resample(), A.last_resample()):
            np.testing.assert_array_equal(x, y)
    # one contract for every kind: once a sensed cycle has run the host-fed calls refuse, and the switch stays on
    U, I = pkg.capi.ERR_UNSUPPORTED, pkg.capi.ERR_INVALID
    w0 = A.get_weights().copy()
    _raises(pkg, U, lambda: A.batch_fastslam_cycle_async(True, Zs, normalize=True), "sensed cycle")
    _raises(pkg, U, lambda: A.resample_async(nz, STEPS + 1), "sensed cycle")
    _raises(pkg, I, lambda: A.serve_sensor(False), "sensed cycle")
    _raises(pkg, I, lambda: A.fastslam_cycle_sensed_async(True), "rfsgpu_batch_sense_async")      # no fresh sense call
    _raises(pkg, U, lambda: A.cycle_sensed_async(True), "rfsgpu_batch_fastslam_cycle_sensed_async")
    np.testing.assert_array_equal(A.get_weights(), w0)
    for bt in (A, B, A_free, A_small):
        bt.close()


RUN_K = 40


def _run_setup(pkg, seeds=(11, 12, 13), sensor=True, log=True, motion=True):
    """3 FastSLAM filters of 32 particles with different Pd and clutter; truth of RUN_K steps of which the first 10 are pinned (so
    both the pinned and the free propagation run) and the first 2 stand still."""
    sim = pkg.sim2d_driver
    base = dict(sim.C1_FASTSLAM_SIM, kmax=RUN_K, n_landmarks=10, eff_n=24.0)
    Ps = [dict(base, Pd=0.99, clutter=1e-4), dict(base, Pd=0.7, clutter=5e-3, eff_n=16.0), dict(base, Pd=0.9, clutter=1e-3)]
    batch = pkg.FastSLAMBatch(3, 32, gm_capacity=256)
    for b, P in enumerate(Ps):
        sim.configure_fastslam_batch_filter(batch, b, P)
        Q = np.array([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2
        if motion or b != 1:
            batch.set_motion_odometry(b, Q, seeds[b])
        batch.set_resampling(b, P["eff_n"], 0.75)
        c = sim.truth_config(P, b)
        c.n_still, c.n_pinned = 2, 10
        batch.set_truth(b, c, seeds[b])
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
    from test_batch_truth import _same_state, _state
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    A, Ps, truth = _run_setup(pkg)
    A.run_truth_async(1, RUN_K, True, *consts)
    sA, logA, scanA = _state(A), A.error_log_read(), A.last_scan()
    assert logA.shape == (RUN_K - 1, 3) and sA["sizes"].max() > 0
    # B: the per-step calls from Python, fed with what get_truth returned
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
        B.fastslam_cycle_sensed_async(True, normalize=True)
        B.resample_sensed_async(k)
        B.step_error_async(np.array([k * P["dt"] for P in Ps]), gt[k], *consts)
    _same_state(sA, _state(B), "run call against per-step calls")
    assert logA.tobytes() == B.error_log_read().tobytes()
    for za, zb in zip(scanA, B.last_scan()):
        np.testing.assert_array_equal(_bits(za), _bits(zb))
    # two calls give what one call gives; so does a run that logs nothing, for the state
    Cc, _, _ = _run_setup(pkg)
    Cc.run_truth_async(1, 17, True, *consts)
    Cc.run_truth_async(17, RUN_K, True, *consts)
    _same_state(sA, _state(Cc), "two calls against one")
    assert Cc.error_log_read().tobytes() == logA.tobytes()
    D, _, _ = _run_setup(pkg, log=False)
    D.run_truth_async(1, 17)
    D.run_truth_async(17, RUN_K)
    _same_state(sA, _state(D), "without the error log")
    # refusals: nothing is enqueued, the state stays
    I = pkg.capi.ERR_INVALID
    for kw, args, needles in ((dict(sensor=False), (1, RUN_K), ("filter 2", "rfsgpu_batch_set_sensor")),
                              (dict(motion=False), (1, RUN_K), ("filter 1", "rfsgpu_batch_set_motion_odometry")),
                              (dict(log=False), (1, RUN_K, True) + consts, ("rfsgpu_error_log_create",))):
        E, _, _ = _run_setup(pkg, **kw)
        s0 = _state(E)
        _raises(pkg, I, lambda: E.run_truth_async(*args), "batch_run_truth", *needles)
        _same_state(s0, _state(E), str(kw))
        E.close()
    for bt in (A, B, Cc, D):
        bt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_truth", [False, True])
def test_the_simulator_loop_with_the_device_sensor(pkg, device_truth):
    """Sim2dBatchRun(FastSLAMBatch, fastslam=True, device_loop=True, device_sensor=True) on data without scans (device_truth: on no
    data at all): no table of scans is built, the last step's sets are the restatement's for the sensors the loop configured, the
    errors are tracked, and a second run gives the same bits."""
    from test_batch_sensed_cycle import _assert_clear_of_the_limits
    sim = pkg.sim2d_driver
    nF, nP, K = 3, 32, 40
    Ps = [dict(sim.C1_FASTSLAM_SIM, kmax=K, n_landmarks=10, Pd=pd, clutter=c) for pd, c in ((0.99, 1e-4), (0.7, 5e-2), (0.9, 1e-2))]      # (a landmark every 4 steps)
    datas = None if device_truth else [sim.generate(P, traj_seed=1 + b, kmax=K, measurements=False) for b, P in enumerate(Ps)]
    seeds = [100 + b for b in range(nF)]
    logs, weights = [], []
    for _ in range(2):
        batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
        if device_truth:
            run = sim.Sim2dBatchRun(batch, None, Ps, seeds, track_errors=True, fastslam=True, device_truth=True, kmax=K)
        else:
            run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, track_errors=True, fastslam=True, device_loop=True, device_sensor=True)
        assert not hasattr(run, "_z") and not hasattr(run, "_nz")
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
        weights.append(_bits(batch.get_weights()))
        batch.close()
    assert logs[0] == logs[1]
    np.testing.assert_array_equal(weights[0], weights[1])
