"""The device truth of a filter batch (include/rfsgpu.h [truth]; csrc/batch_truth.h): rfsgpu_batch_set_truth / _generate_truth /
_get_truth against the numpy restatement of tests/support/truth_reference.py, the restatement's step rules against
sim2d_driver.generate, rfsgpu_batch_run_truth_async against the per-step calls it stands for, and the refusals of the section."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import truth_reference as tr

TRUTH_SYMBOLS = ["rfsgpu_batch_set_truth", "rfsgpu_batch_generate_truth", "rfsgpu_batch_get_truth", "rfsgpu_batch_run_truth_async"]
SHAPES = [(3000, 3000, 20, 50), (120, 3000, 20, 50), (130, 130, 20, 50), (3001, 3001, 20, 50), (60, 60, 3, 60)]      # (K, k_full, n_segments, n_landmarks)
KS = (2, 52, 65, 130, 300)
SEEDS = (0xC0FFEE, 0x1234567890ABCDEF, 77)
TOL = 1e-10       # what tests/test_batch_device_loop.py allows one propagation call and tests/test_batch_sensor.py one scan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


def _configs(sim, i):
    """Three generation configurations for the i-th entry of KS: 0 -- the shipped keys with min_dx = 0.999 max_dx (64 redraws fail with
    probability 0.94 per segment: the fall-back runs); 1 -- spacing 6 from k_full 300 (catch-up segments from step 51), a landmark every
    6 steps, min_dx = 0.9 max_dx (several attempts), a sideways displacement; 2 -- three segments, n_landmarks 0 or 1 in turn."""
    c0 = dict(sim.C1_SIM, min_dx=0.999 * sim.C1_SIM["max_dx"])
    c1 = dict(sim.C1_SIM, kmax=300, n_segments=50, n_landmarks=50, min_dx=0.9 * sim.C1_SIM["max_dx"], max_dy=0.05, vardx=0.001, vardz=0.004)
    c2 = dict(sim.C1_SIM, kmax=300, n_segments=3, n_landmarks=i % 2, rmax=3.0, rmin=0.25)
    return [c0, c1, c2]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_truth_section_and_the_library_exports_it(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    assert "[truth]" in head
    sec = txt.index("---- [truth]")
    assert txt.index("---- [sensor]") < sec
    for s in TRUTH_SYMBOLS:
        assert s not in core, s
        assert sec < txt.index(s + "("), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    m = re.search(r"#define RFSGPU_TRUTH_MAX_STEPS\s+(\d+)\b", txt)
    assert m and int(m.group(1)) >= 3000 and int(m.group(1)) == pkg.capi.TRUTH_MAX_STEPS
    assert "typedef struct rfsgpu_truth_config" in txt[sec:]
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in TRUTH_SYMBOLS:
        assert hasattr(lib, s), s
    for m in ("set_truth", "generate_truth", "get_truth", "run_truth_async"):
        assert callable(getattr(pkg.capi.CBatch, m))
    c = pkg.sim2d_driver.truth_config(pkg.sim2d_driver.C1_SIM)
    want = tr.config(pkg.sim2d_driver.C1_SIM)
    for k, v in want.items():
        assert (list(getattr(c, k)) if k == "var_odo" else getattr(c, k)) == v, k


def _disp_change_steps(sim, gt):
    """The steps at which generate() drew a new displacement, from its poses: the displacement in the frame of the previous pose."""
    d = gt[1:, :2] - gt[:-1, :2]
    c, s = np.cos(gt[:-1, 2]), np.sin(gt[:-1, 2])
    loc = np.column_stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], _wrap(gt[1:, 2] - gt[:-1, 2])])       # loc[k - 1] = disp[k]
    return [k for k in range(2, gt.shape[0]) if np.abs(loc[k - 1] - loc[k - 2]).max() > 1e-9]


@pytest.mark.parametrize("K,k_full,n_seg,n_lm", SHAPES)
def test_restated_segment_and_landmark_steps_are_those_of_generate(pkg, K, k_full, n_seg, n_lm):
    sim = pkg.sim2d_driver
    P = dict(sim.C1_SIM, kmax=k_full, n_segments=n_seg, n_landmarks=n_lm)
    c = tr.config(P)
    d = sim.generate(P, traj_seed=1, kmax=K, measurements=False)
    starts = tr.segment_start_steps(K, c)
    assert _disp_change_steps(sim, d["gt"]) == starts
    assert len(d["landmarks"]) == len(tr.landmark_steps(K, c))
    # ... and the restatement's own displacements change exactly there
    disp, _ = tr.displacements(min(K, 400), c, 5)
    assert [k for k in range(1, len(disp)) if np.any(disp[k] != disp[k - 1])] == [k for k in starts if k < len(disp)]
    if (K, k_full) == (130, 130):
        assert starts[:12] == list(range(51, 62)) + [66]              # spacing 6: one catch-up segment per step from 51 on
    if K == 3001:
        assert len(d["landmarks"]) == 51
    if K == 60:
        assert tr.landmark_steps(K, c) == list(range(1, 60))           # landmark spacing 1


def test_the_redraw_fall_back_is_a_pure_function_of_the_draws():
    c = dict(dt=0.1, max_dx=0.3, min_dx=0.1)
    low = np.linspace(0.0, 0.3, 64)                    # every u max_dx dt below min_dx dt
    assert tr.dx_from_draws(low, c) == ((0.1 + 0.3 * (0.3 - 0.1)) * 0.1, 64, True)                       # the LAST draw, mapped
    first = low.copy()
    first[0] = 0.5
    assert tr.dx_from_draws(first, c) == (0.5 * 0.3 * 0.1, 1, False)
    late = low.copy()
    late[63] = 1.0 / 3.0 + 1e-9
    dx, n, fell = tr.dx_from_draws(late, c)
    assert (n, fell) == (64, False) and dx == late[63] * 0.3 * 0.1
    # the configurations of the GPU test: the fall-back runs, and several attempts are needed
    P = dict(kmax=3000, n_segments=20, n_landmarks=50, dt=0.1, max_dx=0.3, max_dy=0.0, max_dz=0.5, min_dx=0.999 * 0.3, vardx=0, vardy=0, vardz=0, rmax=2.5, rmin=0.5)
    _, info = tr.displacements(300, tr.config(P), SEEDS[0])
    assert any(fell for _, fell in info.values())
    for s, (n, fell) in info.items():
        (dx, _, _), _ = tr.segment_draws(s, tr.config(P), SEEDS[0])
        assert 0.999 * 0.3 * 0.1 * (1 - 1e-15) <= dx < 0.3 * 0.1 and (fell or n <= 64), (s, dx, n, fell)
    _, info = tr.displacements(300, tr.config(dict(P, kmax=300, n_segments=50, min_dx=0.9 * 0.3)), SEEDS[1])
    assert max(n for n, _ in info.values()) > 3 and len(info) > 30


def test_the_chosen_seeds_keep_the_restated_ranges_off_the_limits(pkg):
    """The condition of the first-seen test, on the restatement alone: no true range within 1e-9 of rmin or rmax."""
    sim = pkg.sim2d_driver
    seen_any = False
    for i, K in enumerate(KS):
        for P, seed in zip(_configs(sim, i), SEEDS):
            r = tr.generate(K, tr.config(P), seed)
            assert r["margin"] > 1e-9, (K, seed, r["margin"])
            seen_any |= bool(len(r["first_seen"]) and (r["first_seen"] > 0).any() and r["n_det_max"] > 0)
    assert seen_any


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _generate(pkg, batch, Ps, seeds, K, quiet=False):
    sim = pkg.sim2d_driver
    for b, (P, s) in enumerate(zip(Ps, seeds)):
        c = sim.truth_config(P, b)
        if quiet:
            c.var_odo[0] = c.var_odo[1] = c.var_odo[2] = 0.0
        batch.set_truth(b, c, s)
    batch.generate_truth(K)
    return [batch.get_truth(b) for b in range(len(Ps))]


@pytest.mark.gpu
def test_generated_truth_matches_the_restatement(pkg):
    """Largest deviation of the accumulated trajectory from the restatement's own chain seen on an MI355X: see DESIGN (device truth)."""
    sim = pkg.sim2d_driver
    batch = pkg.FilterBatch(3, 4, gm_capacity=16)
    worst = 0.0
    for i, K in enumerate(KS):
        Ps = _configs(sim, i)
        dev = _generate(pkg, batch, Ps, SEEDS, K)
        quiet = _generate(pkg, batch, Ps, SEEDS, K, quiet=True)       # var_odo 0: the odometry IS the displacement
        for b, (P, seed) in enumerate(zip(Ps, SEEDS)):
            c = tr.config(P)
            d, q = dev[b], quiet[b]
            tag = f"K {K} filter {b}"
            np.testing.assert_array_equal(_bits(d["gt"]), _bits(q["gt"]), err_msg=tag)              # the poses do not depend on the odometry noise
            np.testing.assert_array_equal(_bits(d["landmarks"]), _bits(q["landmarks"]), err_msg=tag)
            disp, info = tr.displacements(K, c, seed)
            np.testing.assert_array_equal(_bits(q["odom"]), _bits(disp), err_msg=tag + ": dx, dy, dz")   # products only: bit-equal
            assert [k for k in range(1, K) if np.any(q["odom"][k] != q["odom"][k - 1])] == tr.segment_start_steps(K, c), tag
            ks = tr.landmark_steps(K, c)
            assert len(d["landmarks"]) == len(ks), tag
            assert np.all(d["gt"][0] == 0) and np.all(d["odom"][0] == 0), tag
            # the chain, link by link, on the device's own poses
            link = sim.odometry_step(d["gt"][:-1], disp[1:])
            err = d["gt"][1:] - link
            err[:, 2] = _wrap(err[:, 2])
            assert np.all(np.abs(err) <= TOL + TOL * np.abs(link)), (tag, np.abs(err).max())
            np.testing.assert_allclose(d["odom"], tr.odometry(disp, c, seed), rtol=TOL, atol=TOL, err_msg=tag)
            np.testing.assert_allclose(d["landmarks"], tr.landmarks(d["gt"], c, seed), rtol=TOL, atol=TOL, err_msg=tag)
            # the accumulated trajectory against the restatement's own chain
            acc = d["gt"] - tr.trajectory(disp)
            acc[:, 2] = _wrap(acc[:, 2])
            dev_max = float(np.abs(acc).max())
            print(f"{tag}: largest deviation of the accumulated trajectory {dev_max:.3e} (bound {(K - 1) * TOL:.1e}), attempts {sorted({n for n, _ in info.values()})}")
            assert dev_max <= (K - 1) * TOL, tag
            worst = max(worst, dev_max)
        if K >= 130:
            assert any(fell for _, fell in tr.displacements(K, tr.config(Ps[0]), SEEDS[0])[1].values())      # the fall-back ran in filter 0
    print(f"largest deviation of any accumulated trajectory: {worst:.3e}")


@pytest.mark.gpu
def test_first_seen_times_and_n_det_max_are_exact(pkg):
    sim = pkg.sim2d_driver
    batch = pkg.FilterBatch(3, 4, gm_capacity=16)
    some = False
    for i, K in enumerate(KS):
        Ps = _configs(sim, i)
        for b, (P, d) in enumerate(zip(Ps, _generate(pkg, batch, Ps, SEEDS, K))):
            c = tr.config(P)
            fs, ndm, margin = tr.first_seen_and_det_max(d["gt"], d["landmarks"], c)
            assert margin > 1e-9, (K, b, margin)            # the condition, on the device's own poses and landmarks
            np.testing.assert_array_equal(_bits(d["first_seen"]), _bits(fs), err_msg=f"K {K} filter {b}")
            np.testing.assert_array_equal(_bits(d["first_seen"]), _bits(sim.first_seen_times(d, P)), err_msg=f"K {K} filter {b}")
            assert d["n_det_max"] == ndm, (K, b)
            assert sim.sensor_max_nz_of(d["n_det_max"], P) == sim.sensor_max_nz(d, P)
            some |= ndm > 1 and bool((fs > 0).any())
    assert some


@pytest.mark.gpu
def test_truth_does_not_depend_on_the_place_and_a_new_generation_replaces_the_tables(pkg):
    sim = pkg.sim2d_driver
    Ps = _configs(sim, 0)
    three = pkg.FilterBatch(3, 4, gm_capacity=16)
    one = pkg.FastSLAMBatch(1, 6, gm_capacity=16)                      # (set / generate / get serve any kind of batch)
    K = 130
    d3 = _generate(pkg, three, Ps, SEEDS, K)
    d1 = _generate(pkg, one, Ps[2:], SEEDS[2:], K)[0]
    for key in ("gt", "odom", "landmarks", "first_seen"):
        np.testing.assert_array_equal(_bits(d1[key]), _bits(d3[2][key]), err_msg=key)
    assert d1["n_det_max"] == d3[2]["n_det_max"]
    # other seeds: other tables
    e3 = _generate(pkg, three, Ps, [s + 1 for s in SEEDS], K)
    for b in range(3):
        assert np.any(e3[b]["odom"] != d3[b]["odom"]) and np.any(e3[b]["gt"][60:] != d3[b]["gt"][60:]), b
    # a shorter generation: the getter writes its rows and no row of the old tables
    f3 = _generate(pkg, three, Ps, SEEDS, 52)
    for b in range(3):
        np.testing.assert_array_equal(_bits(f3[b]["odom"]), _bits(d3[b]["odom"][:52]))
        gt, od = np.full((K, 3), np.nan), np.full((K, 3), np.nan)
        lm, fs = np.zeros((pkg.capi.SENSOR_MAX_LANDMARKS, 2)), np.zeros(pkg.capi.SENSOR_MAX_LANDMARKS)
        n, nd = C.c_int(-1), C.c_int(-1)
        three._call("batch_get_truth", C.c_int(b), three._ptr(gt), three._ptr(od), three._ptr(lm), three._ptr(fs), C.byref(n), C.byref(nd))
        assert np.isnan(gt[52:]).all() and np.isnan(od[52:]).all() and not np.isnan(gt[:52]).any() and not np.isnan(od[:52]).any()
        np.testing.assert_array_equal(_bits(gt[:52]), _bits(d3[b]["gt"][:52]))
        assert n.value == len(tr.landmark_steps(52, tr.config(Ps[b])))
    three._call("batch_get_truth", C.c_int(0), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None))


RUN_K = 130


def _run_setup(pkg, seeds=(11, 12, 13), sensor=True, log=True, ground_truth=True):
    """nF = 3 filters of 16 particles, gm_capacity 32, different Pd and clutter, the third without landmarks; truth of RUN_K steps."""
    sim = pkg.sim2d_driver
    base = dict(sim.C1_SIM, kmax=RUN_K, n_landmarks=10, eff_n=12.0)
    Ps = [dict(base, Pd=0.99, clutter=1e-4), dict(base, Pd=0.7, clutter=5e-3, eff_n=8.0), dict(base, Pd=0.9, clutter=1e-3, n_landmarks=0)]
    batch = pkg.FilterBatch(3, 16, gm_capacity=32)
    for b, P in enumerate(Ps):
        sim.configure_batch_filter(batch, b, P)
        Q = np.array([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2
        batch.set_motion_odometry(b, Q, seeds[b])
        batch.set_resampling(b, P["eff_n"], 0.75)
        batch.set_truth(b, sim.truth_config(P, b), seeds[b])
    batch.generate_truth(RUN_K)
    truth = [batch.get_truth(b) for b in range(3)]
    for b, (P, d) in enumerate(zip(Ps, truth)):
        if sensor:
            batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                             max_nz=sim.sensor_max_nz_of(d["n_det_max"], P), seed=seeds[b])
        if ground_truth:
            batch.set_ground_truth(d["landmarks"], d["first_seen"], filter=b)
    if log:
        batch.error_log_create(RUN_K)
    return batch, Ps, truth


def _state(batch):
    s = dict(w=batch.get_weights(), x=batch.get_poses(), cov=batch.get_pose_covs(), sizes=batch.gm_sizes(), counts=batch.resample_counts(),
             masks=batch.get_unused_masks())
    s["id"], s["parent"] = batch.get_particle_ids()
    for i in range(batch.n):
        for q, a in enumerate(batch.export_gm(i)):
            s[f"gm{i}_{q}"] = a
    return s


def _same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k}"


@pytest.mark.gpu
def test_the_run_call_equals_the_per_step_calls(pkg):
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    A, Ps, truth = _run_setup(pkg)
    A.run_truth_async(1, RUN_K, True, *consts)
    sA, logA, scanA = _state(A), A.error_log_read(), A.last_scan()
    assert logA.shape == (RUN_K - 1, 3)
    for b, P in enumerate(Ps):
        np.testing.assert_array_equal(_bits(logA["t"][:, b]), _bits(np.arange(1, RUN_K) * P["dt"]))      # t[k] = (double) k * dt, bit for bit
    assert sA["counts"].sum() > 0 and sA["sizes"][:32].max() > 0 and len(truth[2]["landmarks"]) == 0
    # B: the existing per-step calls from Python, fed with what get_truth returned
    B, _, truthB = _run_setup(pkg)
    gt = np.ascontiguousarray(np.stack([d["gt"] for d in truthB], axis=1))
    od = np.ascontiguousarray(np.stack([d["odom"] for d in truthB], axis=1))
    for b in range(3):
        np.testing.assert_array_equal(_bits(truthB[b]["gt"]), _bits(truth[b]["gt"]))
    pin = np.ones(3, dtype=np.uint8)
    for k in range(1, RUN_K):
        if k <= 100:
            B.propagate_async(od[k], k, pin=pin, pin_pose=gt[k])
        else:
            B.propagate_async(od[k], k)
        B.sense_async(gt[k], k)
        B.cycle_sensed_async(True, normalize=True)
        B.resample_sensed_async(k)
        B.step_error_async(np.array([k * P["dt"] for P in Ps]), gt[k], *consts)
    _same_state(sA, _state(B), "run call against per-step calls")
    logB = B.error_log_read()
    assert logA.tobytes() == logB.tobytes()
    for za, zb in zip(scanA, B.last_scan()):
        np.testing.assert_array_equal(_bits(za), _bits(zb))
    # two calls give what one call gives; so does a run that logs nothing, for the state
    Cc, _, _ = _run_setup(pkg)
    Cc.run_truth_async(1, 60, True, *consts)
    Cc.run_truth_async(60, RUN_K, True, *consts)
    _same_state(sA, _state(Cc), "two calls against one")
    assert Cc.error_log_read().tobytes() == logA.tobytes()
    D, _, _ = _run_setup(pkg, log=False, ground_truth=False)
    D.run_truth_async(1, 60)
    D.run_truth_async(60, 60)                           # an empty range: nothing
    D.run_truth_async(60, RUN_K)
    _same_state(sA, _state(D), "without the error log")
    # the driver's form: one call, the same bits again
    E = pkg.FilterBatch(3, 16, gm_capacity=32)
    run = sim.Sim2dBatchRun(E, None, Ps, [11, 12, 13], track_errors=True, device_truth=True, kmax=RUN_K)
    for b, P in enumerate(Ps):
        E.set_resampling(b, P["eff_n"], 0.75)
    run.run()
    assert run.errors().tobytes() == logA.tobytes()


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


@pytest.mark.gpu
def test_the_truth_section_refuses_with_the_state_and_the_tables_untouched(pkg):
    sim, capi = pkg.sim2d_driver, pkg.capi
    I, U, CAP = capi.ERR_INVALID, capi.ERR_UNSUPPORTED, capi.ERR_CAPACITY
    batch, Ps, truth = _run_setup(pkg, sensor=False, log=False, ground_truth=False)
    w0 = batch.get_weights().copy()

    def untouched():
        np.testing.assert_array_equal(_bits(batch.get_weights()), _bits(w0))
        for b in range(3):
            d = batch.get_truth(b)
            for key in ("gt", "odom", "landmarks", "first_seen"):
                np.testing.assert_array_equal(_bits(d[key]), _bits(truth[b][key]))

    good = sim.truth_config(Ps[0])
    nan, inf = float("nan"), float("inf")
    bad = [("dt", nan), ("dt", -0.1), ("max_dx", inf), ("max_dy", -1.0), ("max_dz", nan), ("min_dx", -0.1), ("rmax", nan), ("rmin", -0.5),
           ("var_odo", (0.1, -0.1, 0.1)), ("var_odo", (nan, 0.1, 0.1)), ("k_full", -5), ("n_still", -1), ("n_pinned", -1), ("n_landmarks", -1),
           ("min_dx", 0.31), ("rmin", 2.5), ("rmin", 3.0), ("n_segments", 0), ("n_segments", RUN_K + 1), ("n_landmarks", RUN_K + 1)]
    for name, v in bad:
        c = sim.truth_config(Ps[0])
        if name == "var_odo":
            for q in range(3):
                c.var_odo[q] = v[q]
        else:
            setattr(c, name, v)
        _raises(pkg, I, lambda: batch.set_truth(0, c, 1), "batch_set_truth")
    many = sim.truth_config(dict(Ps[0], kmax=4000, n_landmarks=4000))       # spacing 1: 3999 landmarks could be placed
    _raises(pkg, I, lambda: batch.set_truth(0, many, 1), "RFSGPU_SENSOR_MAX_LANDMARKS")
    _raises(pkg, I, lambda: batch.set_truth(3, good, 1), "filter")
    _raises(pkg, I, lambda: batch.set_truth(0, None, 1), "null")
    # n_steps of 1, above the cap, above a filter's k_full
    for n in (1, 0, capi.TRUTH_MAX_STEPS + 1):
        _raises(pkg, I, lambda: batch._call("batch_generate_truth", C.c_int(n)), "RFSGPU_TRUTH_MAX_STEPS")
    _raises(pkg, I, lambda: batch._call("batch_generate_truth", C.c_int(RUN_K + 1)), "filter 0", "k_full")
    untouched()
    # a run outside [1, n_steps]; a filter without a sensor; track_errors without ground truth / log
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    for b in (0, 2):
        P, d = Ps[b], truth[b]
        batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"], seed=3)
    _raises(pkg, I, lambda: batch.run_truth_async(1, 5), "filter 1", "rfsgpu_batch_set_sensor")
    P, d = Ps[1], truth[1]
    batch.set_sensor(1, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"], seed=3)
    for rng in ((0, 5), (5, 4), (1, RUN_K + 1), (-1, 2)):
        _raises(pkg, I, lambda: batch.run_truth_async(*rng), "k_from")
    _raises(pkg, I, lambda: batch.run_truth_async(1, 5, True, *consts), "filter 0", "rfsgpu_set_ground_truth")
    batch.set_ground_truth(truth[0]["landmarks"], truth[0]["first_seen"], filter=0)
    _raises(pkg, I, lambda: batch.run_truth_async(1, 5, True, *consts), "filter 1", "rfsgpu_set_ground_truth")
    for b in (1, 2):
        batch.set_ground_truth(truth[b]["landmarks"], truth[b]["first_seen"], filter=b)
    _raises(pkg, I, lambda: batch.run_truth_async(1, 5, True, *consts), "rfsgpu_error_log_create")
    batch.error_log_create(3)
    _raises(pkg, CAP, lambda: batch.run_truth_async(1, 5, True, *consts), "error log")
    assert len(batch.error_log_read()) == 0
    untouched()
    # generating with an unset filter names the lowest one, and running before generating is refused
    fresh = pkg.FilterBatch(3, 4, gm_capacity=16)
    f0 = fresh.get_weights().copy()
    _raises(pkg, I, lambda: fresh.run_truth_async(1, 2), "rfsgpu_batch_generate_truth", "filter 0")
    _raises(pkg, I, lambda: fresh._call("batch_get_truth", C.c_int(0), *([C.c_void_p(None)] * 6)), "rfsgpu_batch_generate_truth")
    fresh.set_truth(0, good, 1)
    fresh.set_truth(2, good, 1)
    _raises(pkg, I, lambda: fresh.generate_truth(20), "filter 1", "rfsgpu_batch_set_truth")
    _raises(pkg, I, lambda: fresh.run_truth_async(1, 2), "rfsgpu_batch_generate_truth")
    fresh.set_truth(None, good, 1)
    fresh.generate_truth(20)
    np.testing.assert_array_equal(_bits(fresh.get_weights()), _bits(f0))
    # the run call on a FastSLAM or multi-hypothesis batch; set / generate / get serve them
    fs = pkg.FastSLAMBatch(2, 4, gm_capacity=16)
    fs.configure_fastslam(0, sim.fastslam_config(fs))
    mh = pkg.MHFastSLAMBatch(2, 4, gm_capacity=16)
    for f, what in ((fs, "FastSLAM"), (mh, "multi-hypothesis")):
        v0 = f.get_weights().copy()
        f.set_truth(None, good, 7)
        f.generate_truth(60)
        d = f.get_truth(1)
        assert d["gt"].shape == (60, 3) and len(d["landmarks"]) == len(tr.landmark_steps(60, tr.config(Ps[0])))
        _raises(pkg, U, lambda: f.run_truth_async(1, 5), what)
        np.testing.assert_array_equal(_bits(f.get_weights()), _bits(v0))
    # set_truth (and the rest of the section) on an ordinary handle or a group shard
    single = pkg.RBPHDFilter(8, gm_capacity=16)
    group = pkg.FilterGroup(16, [0, 0], gm_capacity=16)
    for f, what in ((single, "ordinary handle"), (group.shards[0], "shard")):
        v0 = f.get_weights().copy()
        _raises(pkg, U, lambda: f._call("batch_set_truth", C.c_int(-1), C.byref(good), C.c_ulonglong(1)), what)
        _raises(pkg, U, lambda: f._call("batch_generate_truth", C.c_int(20)), what)
        _raises(pkg, U, lambda: f._call("batch_get_truth", C.c_int(0), *([C.c_void_p(None)] * 6)), what)
        _raises(pkg, U, lambda: f._call("batch_run_truth_async", C.c_int(1), C.c_int(2), C.c_int(0), C.c_double(0.75), C.c_double(0.2), C.c_double(1.0)), what)
        np.testing.assert_array_equal(f.get_weights(), v0)
    group.close()
