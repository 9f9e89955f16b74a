"""The sensed cycle of a filter batch (include/rfsgpu.h [sensor]): sense -> cycle_sensed -> resample_sensed on one handle against the
host-fed rfsgpu_batch_cycle_async / rfsgpu_batch_resample_async on a twin that is handed the first handle's scans, bit for bit."""
import numpy as np
import pytest

from tests.support import sensor_reference as sr

NF, NP, STEPS, QUIET = 5, 65, 12, 4
DENSE = 12.0 / (2 * np.pi * 2.0)          # clutter intensity whose mean over [0.5, 2.5] is 12
R_SENSOR = np.diag([5e-4, 5e-5])
SMALL_BOUND = 48                          # the second max_nz bound (no restated scan reaches it; last_cycle_lds shows that it is another launch)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(pkg, scens):
    """Scenario maps as tests/test_batch_device_loop.py::_scenario_batches builds them (room for the clutter's births)."""
    from test_filter_batch import _configure_from_scenario
    batch = pkg.FilterBatch(NF, NP, gm_capacity=512)
    batch.set_poses(np.vstack([s["poses"] for s in scens]), np.vstack([np.tile(np.asarray(s["pose_cov"], dtype=np.float64).ravel(), (NP, 1)) for s in scens]))
    batch.set_weights(np.concatenate([s["particle_w"] for s in scens]))
    for b, s in enumerate(scens):
        _configure_from_scenario(pkg.capi, batch, b, s["params"])
        for i in range(NP):
            batch.import_gm(b * NP + i, s["w"][i], s["mean"][i], s["cov"][i])
        batch.set_motion_odometry(b, [2e-5, 2e-5, 1e-5], 500 + b)
        batch.set_resampling(b, 0.98 * NP, 0.98)
    return batch


def _sensors(scens):
    """Filter 0 never sees anything (Pd 0, no clutter); filter 1 stands far from its landmarks for the first QUIET steps; filter 2 has
    dense clutter; 3 and 4 are ordinary."""
    out = []
    for b, s in enumerate(scens):
        out.append(dict(R=R_SENSOR, Pd=[0.0, 0.9, 0.4, 0.95, 0.6][b], clutter=[0.0, 0.0, DENSE, 1e-4, 0.05][b], rmax=2.5, rmin=0.5,
                        lm=s["gt"][: [40, 40, 40, 25, 40][b]], seed=9000 + b))
    return out


def _set_sensors(batch, sensors, max_nz):
    for b, s in enumerate(sensors):
        batch.set_sensor(b, s["R"], s["Pd"], s["clutter"], s["rmax"], s["rmin"], s["lm"], max_nz=max_nz, seed=s["seed"])


def _inputs():
    rng = np.random.default_rng(4)
    gt = np.zeros((STEPS + 1, NF, 3))
    u = np.zeros((STEPS + 1, NF, 3))
    for k in range(1, STEPS + 1):
        u[k] = rng.uniform(-1, 1, (NF, 3)) * [0.01, 0.004, 0.01]
        gt[k] = gt[k - 1] + u[k]
    gt[1:QUIET + 1, 1, :2] += 50.0
    return gt, u


def _state(bt):
    return dict(w=_bits(bt.get_weights()), sizes=bt.gm_sizes(), masks=bt.get_unused_masks(), poses=_bits(bt.get_poses()),
                ids=[np.asarray(v) for v in bt.get_particle_ids()], occured=bt.batch_resample_occured(),
                gm=[[_bits(x) for x in bt.export_gm(i)] for i in range(bt.n)])


def _assert_clear_of_the_limits(info, rmin, rmax, what):
    for lim in (rmin, rmax):
        assert info["ranges"].size == 0 or np.abs(info["ranges"] - lim).min() > 1e-9, what


def _assert_same(sa, sb, what):
    for key in ("w", "sizes", "masks", "poses", "occured"):
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{what}: {key}")
    for x, y in zip(sa["ids"], sb["ids"]):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: particle ids")
    for i, (ga, gb) in enumerate(zip(sa["gm"], sb["gm"])):
        for x, y in zip(ga, gb):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: mixture of slot {i}")


@pytest.mark.gpu
def test_sensed_cycle_equals_the_host_fed_cycle_on_the_same_scans(pkg, sc):
    scens = [sc.make_scenario(NP, 40, 10, seed=901 + b) for b in range(NF)]
    sensors = _sensors(scens)
    gt, u = _inputs()
    # what the sensors will deliver, by the restatement: the premises of this test
    restated = [[sr.scan(gt[k, b], s["lm"], s["R"], s["Pd"], s["clutter"], s["rmin"], s["rmax"], s["seed"], k) for b, s in enumerate(sensors)]
                for k in range(1, STEPS + 1)]
    counts = np.array([[len(Z) for Z, _ in row] for row in restated])
    # (the exact comparison of the device's counts with these rests on no decision hanging on a range nearer than 1e-9 to a limit --
    #  ten times the bound on device-against-numpy values, as in tests/test_batch_sensor.py)
    for k, row in enumerate(restated):
        for (_, info), s in zip(row, sensors):
            _assert_clear_of_the_limits(info, s["rmin"], s["rmax"], (k + 1, s["seed"]))
    assert counts[:, 0].max() == 0                                                    # one filter never sees anything
    assert counts[:QUIET, 1].max() == 0 and counts[QUIET, 1] > 0                      # one goes from empty scans to non-empty ones
    assert counts[:, 2].min() >= 12 and counts.max() < SMALL_BOUND                    # dense clutter; both bounds hold every scan
    A, B, A_free, A_small = (_batch(pkg, scens) for _ in range(4))
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
        A.cycle_sensed_async(True, normalize=True)
        A.resample_sensed_async(k)
        A.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        B.propagate_async(u[k], k)
        B.cycle_async(True, Zs, normalize=True)
        B.resample_async(nz, k)
        B.step_error_async(t, gt[k], 0.75, 0.20, 1.0)
        for bt in (A_free, A_small):
            bt.propagate_async(u[k], k)
            bt.sense_async(gt[k], k)
            bt.cycle_sensed_async(True, normalize=True)
            bt.resample_sensed_async(k)
        _assert_same(_state(A), _state(B), f"step {k}")
        la, lb = A.last_resample(), B.last_resample()
        np.testing.assert_array_equal(la[0], lb[0], err_msg=f"step {k}: fired")
        np.testing.assert_array_equal(la[1], lb[1], err_msg=f"step {k}: plan")
        np.testing.assert_array_equal(_bits(la[2]), _bits(lb[2]), err_msg=f"step {k}: N_eff")
        fired_any |= bool(la[0].any())
        went_nonempty |= bool(((last_nz == 0) & (nz > 0) & (k > 1)).any())
        last_nz = nz
    assert fired_any, "no resampling fired: the test does not reach the inheritance after one"
    assert went_nonempty
    np.testing.assert_array_equal(A.resample_counts(), B.resample_counts())
    ea, eb = A.error_log_read(), B.error_log_read()
    assert ea.shape[0] == STEPS and ea.tobytes() == eb.tobytes()
    sa = _state(A)
    _assert_same(sa, _state(A_free), "the free-running handle")
    _assert_same(sa, _state(A_small), f"max_nz {SMALL_BOUND} against 64")
    # (the two bounds did give two launches: the step kernel's LDS block grows with the bound)
    assert 0 < A_small.last_cycle_lds() < A.last_cycle_lds() == A_free.last_cycle_lds()
    for bt in (A_free, A_small):
        for x, y in zip(bt.last_resample(), A.last_resample()):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_the_simulator_loop_with_the_device_sensor(pkg):
    """Sim2dBatchRun(device_loop=True, device_sensor=True) on data without scans: no table of scans is built, the last step's sets are
    the restatement's for the sensors the loop configured, the errors are tracked, and a second run gives the same bits."""
    sim = pkg.sim2d_driver
    nF, nP, K = 3, 32, 40
    Ps = [dict(sim.C1_SIM, kmax=K, Pd=pd, clutter=c) for pd, c in ((0.99, 1e-4), (0.7, 5e-2), (0.9, 1e-2))]      # (kmax = K: a landmark per step)
    datas = [sim.generate(P, traj_seed=1 + b, kmax=K, measurements=False) for b, P in enumerate(Ps)]
    seeds = [100 + b for b in range(nF)]
    logs, weights = [], []
    for _ in range(2):
        batch = pkg.FilterBatch(nF, nP, gm_capacity=256)
        run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, track_errors=True, device_loop=True, device_sensor=True)
        assert not hasattr(run, "_z") and not hasattr(run, "_nz")
        run.run(1, K)
        scans = batch.last_scan()
        for b, (P, d) in enumerate(zip(Ps, datas)):
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
