"""rfsgpu_fastslam_cycle_full_async: the whole FastSLAM::update on the device for either measurement model and with landmark
candidate lists, the motion and static-step calls that enqueue behind pending cycles, and vp_driver.VictoriaParkRun on that route.

The yardstick is the host-stop route on a second handle given the same state, measurements and draws (rfsgpu_fastslam_update + the
host's resampleWithMapCopy): the same kernels on the same inputs in the same order, so states are compared bit for bit -- count,
parents, normalised weights, ordered maps, candidate lists (means, covariances, support and check counts), poses, ids.  What a
kernel launched at max_particles with the count on the device can get wrong is a write beyond the live count: every slot from the
grown count up is planted with a pattern beforehand and read again afterwards (rfsgpu_debug_slot).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import mh_device_cycle_reference as mh
from tests.support import vp_device_cycle_reference as ref

NEVER = ref.NEVER
VP_KW = {"const": dict(n_landmarks=30, n_z=9, seed=91, scan="const"), "ragged": dict(n_landmarks=70, n_z=18, seed=92, scan="ragged")}


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_new_calls_are_exported_with_the_header_s_arguments(pkg):
    pkg.build_mod.build()
    lib = pkg.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfsgpu.h")).read(), flags=re.S)
    want = {
        "rfsgpu_fastslam_cycle_full_async": "rfsgpu_filter *f, int predict, const double *z, int n_z, const double *scan, int n_scan, double u01, int n_init",
        "rfsgpu_fastslam_cycle_counts": "rfsgpu_filter *f, int *n_cycles, int *n_resamplings",
        "rfsgpu_fastslam_cycle_pending": "rfsgpu_filter *f",
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name + " is not declared"
        assert " ".join(m.group(1).split()) == args
        assert name[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    lib.rfsgpu_fastslam_cycle_full_async.restype = C.c_int
    assert lib.rfsgpu_fastslam_cycle_full_async(C.c_void_p(), C.c_int(0), C.c_void_p(), C.c_int(0), C.c_void_p(), C.c_int(0), C.c_double(0.5),
                                                C.c_int(1)) == pkg.capi.ERR_INVALID
    lib.rfsgpu_fastslam_cycle_pending.restype = C.c_int
    assert lib.rfsgpu_fastslam_cycle_pending(C.c_void_p()) == 0


@pytest.mark.parametrize("n", [1, 2, 65])
def test_pose_bookkeeping_under_copies_and_plans_equals_the_plain_loop(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 3))
    nH = rng.integers(1, 4, n)
    grown, parents = mh.host_loop_plan(nH)[:2]
    assert np.array_equal(ref.follow_poses(x, parents), ref.follow_poses_loop(x, parents))
    assert np.array_equal(ref.follow_poses(x, parents)[:n], x)                       # a particle keeps its own slot
    for n_out in sorted({1, n, grown}):
        plan = rng.integers(0, grown, n_out)
        got = ref.follow_poses(x, parents, plan)
        assert got.shape == (n_out, 3) and np.array_equal(got, ref.follow_poses_loop(x, parents, plan))
        assert np.array_equal(got, x[parents[plan]])


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _one_cycle(pkg, sc, scen, hyp, thr, cur_thr):
    """Warm both handles up with one plain update (candidate lists fill), then one update with its tail on each route."""
    n0 = scen["n"]
    cap = n0 * hyp + 1
    host, dev = ref.make_pair(pkg, sc, scen, hyp, thr, cur_thr, cap)
    rz = np.random.default_rng(3)
    ref.warm_up((host, dev), scen["Z"] + rz.normal(0, 1e-3, scen["Z"].shape))
    Z = scen["Z"] + rz.normal(0, 1e-3, scen["Z"].shape)
    host.predict_map()
    assert host.update_and_resample(Z, u01_fn=lambda: 0.25) is False
    grown = host.n
    assert n0 <= grown < cap == dev.max_particles
    ref.poison(dev, grown)
    dev.predict_map()
    assert dev.update_and_resample(Z, u01_fn=lambda: 0.25) is False
    lc = dev.last_cycle
    assert lc["n_after_update"] == lc["n_after_resample"] == grown == dev.n and not lc["fired"]
    assert np.array_equal(lc["parent"], host.parents) and np.array_equal(dev.parents, host.parents)
    a, b = ref.state(host), ref.state(dev)
    ref.assert_same_state(a, b)
    assert host.resampleOccured is False and dev.resampleOccured is False
    ref.assert_poison(dev, grown)
    ncand = sum(len(c[2]) for c in a["cands"])
    host.close(); dev.close()
    return grown, ncand


VP_CASES = [(1, 16, 2, 0, "const"), (1, 1, 4, 1, "ragged"), (63, 3, 2, 0, "ragged"), (63, 1, 1, 0, "const"), (65, 16, 4, 1, "const"),
            (65, 3, 1, 1, "ragged"), (65, 1, 2, 0, "ragged"), (257, 3, 4, 0, "const"), (257, 1, 4, 1, "const"), (257, 3, 2, 1, "ragged"),
            (63, 16, 4, 0, "const"), (65, 3, 4, 0, "ragged")]


@pytest.mark.gpu
@pytest.mark.parametrize("n0,hyp,thr,cur_thr,scan", VP_CASES)
def test_one_victoria_park_cycle_equals_the_host_stop_route(pkg, sc, n0, hyp, thr, cur_thr, scan):
    scen = sc.make_vp_scenario(n_particles=n0, **VP_KW[scan])
    grown, ncand = _one_cycle(pkg, sc, scen, hyp, thr, cur_thr)
    print("vp %s n0 %d hyp %d thr %d/%d: grown %d, candidates %d" % (scan, n0, hyp, thr, cur_thr, grown, ncand))
    if thr > 1 and cur_thr == 0:
        assert ncand > 0, "no landmark candidate was queued: the lists were not exercised"


@pytest.mark.gpu
@pytest.mark.parametrize("n0,hyp,thr,cur_thr", [(1, 16, 2, 0), (63, 3, 4, 1), (65, 16, 4, 0), (65, 1, 2, 0), (257, 3, 2, 1), (257, 1, 4, 0)])
def test_one_2d_cycle_with_candidate_lists_equals_the_host_stop_route(pkg, sc, n0, hyp, thr, cur_thr):
    scen = mh.crowded(sc, n0)
    grown, ncand = _one_cycle(pkg, sc, scen, hyp, thr, cur_thr)
    print("2-D n0 %d hyp %d thr %d/%d: grown %d, candidates %d" % (n0, hyp, thr, cur_thr, grown, ncand))
    if hyp > 1:
        assert grown > n0


@pytest.mark.gpu
def test_the_new_call_serves_what_the_old_one_refuses(pkg, sc):
    """(the old call's refusals themselves: tests/test_mh_fastslam_device_cycle.py::test_refused_configurations_leave_the_state_untouched)"""
    Z3 = np.array([[20.0, 1.2, 0.8], [31.0, 1.9, 0.5]])
    vp = pkg.RBPHDFilter(4, gm_capacity=64, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    with pytest.raises(pkg.capi.EngineError) as e:
        vp.fastslam_cycle_async(Z3, 0.5, 4)
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED
    with pytest.raises(pkg.capi.EngineError) as e:            # the 3-D model with no scan ever set
        vp.fastslam_cycle_full_async(Z3, 0.5, 4)
    assert e.value.status == pkg.capi.ERR_INVALID
    sc.apply_vp_params(vp, sc.VP_PARAMS, np.full(361, 70.0))
    vp.fastslam_cycle_full_async(Z3, 0.5, 4, scan=np.full(361, 60.0))
    assert vp.fastslam_cycle_pending()
    assert vp.n == 4 and not vp.fastslam_cycle_pending()
    vp.close()
    f = pkg.RBPHDFilter(4, gm_capacity=64, max_particles=64)
    scen = mh.crowded(sc, 4)
    sc.load_scenario(f, scen)
    cfg = f.default_fastslam_config()
    cfg.landmarkCandidateMeasurementCountThreshold = 2
    f.set_fastslam_config(cfg)
    with pytest.raises(pkg.capi.EngineError) as e:
        f.fastslam_cycle_async(scen["Z"], 0.5, 4)
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED
    f.fastslam_cycle_full_async(scen["Z"], 0.5, 4)
    assert f.n == 4 and np.array_equal(f.fastslam_last_cycle()["parent"], np.arange(4))
    with pytest.raises(pkg.capi.EngineError) as e:            # a scan needs the Victoria Park model
        f.fastslam_cycle_full_async(scen["Z"], 0.5, 4, scan=np.full(361, 60.0))
    assert e.value.status == pkg.capi.ERR_INVALID
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("resampled", [True, False])
def test_candidates_travel_with_copies_only_after_a_resampling(pkg, ob, sc, resampled):
    """Two consecutive cycles on a multiplying 3-D scenario.  The first either resamples (forced back to n0: the grown count exceeds
    nParticlesMax) or is kept from it; the copies the second one makes carry their parent's candidate list in the first case and
    none in the second (fresh slots).  The host-stop route is driven with rfsgpu_fastslam_set_resample_occured; the oracle follows
    through the same host steps at the tolerances of test_fastslam_victoria_park_model."""
    from tests.test_gpu_parity import _compare_fastslam
    n0, hyp = 6, 3
    scen = sc.make_vp_scenario(n_particles=n0, n_landmarks=12, n_z=8, seed=112, scan="const")
    cap = n0 * hyp * hyp + 1
    host, dev = ref.make_pair(pkg, sc, scen, hyp, 2, 0, cap)
    orc = ob.OracleFilter(n0, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    sc.load_scenario(orc, scen)
    for i in range(n0):
        orc.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
    ocfg = ref.candidate_config(orc.default_fastslam_config(), 2, 0)
    ocfg.maxNDataAssocHypotheses = hyp
    ocfg.maxDataAssocLogLikelihoodDiff = 50.0
    orc.set_fastslam_config(ocfg)
    rz = np.random.default_rng(5)
    Zs = [scen["Z"] + rz.normal(0, 1e-3, scen["Z"].shape) for _ in range(2)]
    for f in (host, dev):
        f.fs_config.nParticlesMax = n0 if resampled else cap        # forced after the first update, or never
    counts, carried = [], 0
    for k, Z in enumerate(Zs):
        if k == 1:
            carried = sum(len(c[2]) for c in ref.state(host)["cands"][:n0])          # what the copies of this update could inherit
            for f in (host, dev):
                f.fs_config.nParticlesMax = cap
        for f in (host, dev):
            f.predict_map()
            assert f.update_and_resample(Z, u01_fn=lambda: 0.37) == (resampled and k == 0)
        # the oracle through the host route's own steps
        orc.predict_map(False)
        orc.fastslam_update(Z)
        assert np.array_equal(orc.particle_parents(), host.parents)
        orc.normalize_weights(orc.weight_sums()[0])
        if resampled and k == 0:
            orc.resample_apply(host.last_resample_plan, n_out=n0)
        orc.fastslam_set_resample_occured(resampled and k == 0)
        counts.append(host.n)
        assert host.n == dev.n == orc.n
        ref.assert_same_state(ref.state(host), ref.state(dev))
        _compare_fastslam(sc, host, orc, host.n)
    print("resampled %s: counts %s" % (resampled, counts))
    par = host.parents
    copies = [s for s in range(len(par)) if par[s] != s]
    assert copies, "the second update made no copies"
    # The rule itself shows only through the two independent statements of it that the states above were held against (the
    # host-stop route under rfsgpu_fastslam_set_resample_occured, and the oracle): after the second update parent and copy have
    # walked different hypotheses.  What is asserted here is that the case had something to tell apart.
    assert carried > 0, "no particle had a candidate list when the second update copied it"
    assert counts == ([n0, n0 * hyp] if resampled else [n0 * hyp, n0 * hyp * hyp])      # (after each cycle's resampling, if any)
    host.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vp", [True, False])
def test_motion_and_static_steps_behind_pending_cycles(pkg, sc, vp):
    """cycle (multiplying), a propagation run of 3 and one of 17 steps (longer than ACKERMAN_RUN_MAX), a single propagation, two static
    steps, a scan, a cycle -- with no synchronising call in between, against the same sequence with rfsgpu_synchronize after every
    call.  The pending flag stays up throughout: none of the calls took the count over (mhc_resolve clears it)."""
    n0, hyp = 5, 3
    scen = sc.make_vp_scenario(n_particles=n0, n_landmarks=12, n_z=8, seed=112, scan="const") if vp else mh.crowded(sc, n0)
    cap = n0 * hyp * hyp + 1
    dm = 3 if vp else 2
    geom = (0.76, 2.83, 3.78, 0.50)
    rng = np.random.default_rng(2)
    u3, u17 = rng.uniform(0.5, 2.0, (3, 2)) * [1.0, 0.05], rng.uniform(0.5, 2.0, (17, 2)) * [1.0, 0.05]
    v3, v17 = np.tile([0.04, 1e-4], (3, 1)), np.tile([0.04, 1e-4], (17, 1))
    q = np.stack([np.eye(dm) * 1e-4, np.eye(dm) * 3e-4])
    Z2 = scen["Z"] + rng.normal(0, 1e-3, scen["Z"].shape)
    out = []
    for wait in (True, False):
        h, f = ref.make_pair(pkg, sc, scen, hyp, 2, 0, cap)
        h.close()
        ref.warm_up((f,), scen["Z"])
        pc = np.tile(np.diag([1e-4, 1e-4, 1e-6]), (n0, 1, 1))
        f.set_poses(scen["poses"], pc)
        if not wait:
            ref.poison(f, out[0]["n"])
        steps = [lambda: f.cycle_async(scen["Z"], 0.3),
                 lambda: f.propagate_ackerman_run_async(u3, v3, np.full(3, 0.025), geom, 7, 0),
                 lambda: f.propagate_ackerman_run_async(u17, v17, np.full(17, 0.025), geom, 7, 3),
                 lambda: f.propagate_ackerman_async(u3[0], v3[0], 0.025, geom, 7, 20),
                 lambda: f.static_steps_async(2, q),
                 lambda: f.set_step_inputs_async(scan=scen["scan"] * 0.99) if vp else None,
                 lambda: f.cycle_async(Z2, 0.6, push_config=False)]
        for step in steps:
            step()
            if wait:
                f.synchronize()
            else:
                assert f.fastslam_cycle_pending(), "a call behind a pending cycle took the particle count over"
        s = ref.state(f)
        s["pose_cov"] = f.get_pose_covs()
        assert not f.fastslam_cycle_pending()
        out.append(s)
        if not wait:
            ref.assert_poison(f, s["n"])
        f.close()
    a, b = out
    print("%s: %d -> %d particles" % ("vp" if vp else "2-D", n0, a["n"]))
    assert a["n"] > n0
    ref.assert_same_state(a, b)
    assert np.array_equal(a["pose_cov"], b["pose_cov"])
    assert not np.array_equal(a["poses"][:n0], scen["poses"])                        # the poses did move


@pytest.mark.gpu
def test_capacity_exact_fit_passes_and_one_more_copy_abandons_what_is_queued(pkg, sc):
    n0, hyp = 4, 4
    scen = mh.crowded(sc, n0)
    geom = (0.76, 2.83, 3.78, 0.50)
    for cap, fits in ((16, True), (15, False)):
        dev = pkg.RBPHDFilter(n0, gm_capacity=64, max_particles=cap)
        sc.load_scenario(dev, scen)
        for i in range(n0):
            dev.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
        cfg = dev.default_fastslam_config()
        cfg.maxNDataAssocHypotheses = hyp
        cfg.maxDataAssocLogLikelihoodDiff = 50.0
        cfg.minUpdatesBeforeResample = NEVER
        cfg.nParticlesMax = cap
        cfg.landmarkCandidateMeasurementCountThreshold = 2
        cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
        dev.set_fastslam_config(cfg)
        before = ref.state(dev)
        dev.fastslam_cycle_full_async(scen["Z"], 0.5, n0)
        dev.propagate_ackerman_run_async([[1.0, 0.02], [1.2, 0.01]], None, [0.025, 0.025], geom, 3, 0)      # queued behind the cycle
        dev.static_steps_async(1, np.eye(2)[None] * 1e-3)
        assert dev.fastslam_cycle_pending()
        if fits:
            dev.synchronize()
            assert dev.n == 16 and dev.fastslam_last_cycle()["n_after_update"] == 16
            assert not np.array_equal(dev.get_poses()[:n0], before["poses"])
        else:
            dev.fastslam_cycle_full_async(scen["Z"], 0.5, n0)
            with pytest.raises(pkg.capi.EngineError) as e:
                dev.synchronize()
            assert e.value.status == pkg.capi.ERR_CAPACITY and "max_particles" in str(e.value)
            dev.synchronize()                                                       # reported once
            ref.assert_same_state(before, ref.state(dev))                           # the poses and maps from before the abandoned cycle
        dev.close()


def _extract():
    return np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))


def _vp_run(pkg, sc, make, n, hyp, n_max, thr, diff, n_messages, **opts):
    f = make()
    P = dict(sc.VP_PARAMS)
    sc.apply_vp_params(f, P, np.full(361, 70.0))
    cfg = f.default_fastslam_config()
    cfg.minLogMeasurementLikelihood = -15.0
    cfg.mapExistencePruneThreshold = -5.0
    cfg.landmarkCandidateMeasurementCountThreshold = thr
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementCheckThreshold = 5
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.maxNDataAssocHypotheses = hyp
    cfg.maxDataAssocLogLikelihoodDiff = diff
    f.set_fastslam_config(cfg)
    return pkg.vp_driver.VictoriaParkRun(f, _extract(), P, seed=5, filter="fastslam", max_hypotheses=hyp, n_particles_max=n_max, **opts).run(n_messages=n_messages)


@pytest.mark.gpu
def test_dataset_extract_single_hypothesis_device_cycle_equals_host_stop_route(pkg, sc):
    """900 messages of the Victoria Park extract, 32 particles, the configuration values of test_victoria_park_dataset_extract_fastslam,
    poses propagated on the device under one seed and one resampling draw per update on both routes."""
    n = 32
    make = lambda: pkg.RBPHDFilter(n, gm_capacity=192, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    host = _vp_run(pkg, sc, make, n, 1, n, 3, 3.0, 900, device_motion=True, draw_every_update=True)
    dev = _vp_run(pkg, sc, make, n, 1, n, 3, 3.0, 900, device_cycle=True)
    print("lidar updates %d, resamplings host %d device %d" % (host.n_lidar, host.n_resamples, dev.n_resamples))
    assert dev.n_lidar == host.n_lidar > 50
    assert dev.n_resamples == host.n_resamples >= 1
    a, b = ref.state(host.f), ref.state(dev.f)
    assert a["sizes"].max() > 3
    ref.assert_same_state(a, b)
    host.f.close(); dev.f.close()


@pytest.mark.gpu
def test_dataset_extract_three_hypotheses_device_cycle_equals_host_stop_route(pkg, ob, sc):
    """900 messages, 16 particles, nParticlesMax 48, likelihood window 3.0, candidate threshold 4: the particle set grows and is
    forced back; the device cycle equals the host-stop route bit for bit.

    The host-stop route against ob.OracleFilter under the same driver (host poses that follow particle_parents() and the plans),
    at the tolerances of test_victoria_park_dataset_extract_fastslam, over 900 messages: measured on its own, the
    host-stop route -- the parent commit's kernels, it runs no new device code -- agrees with the oracle at 300, 600 and 900
    messages (29 / 59 / 89 lidar updates, 14 / 29 / 44 resamplings, all forced, sets grown to 144), so the longest length stands."""
    n = 16
    make = lambda: pkg.RBPHDFilter(n, gm_capacity=192, model=pkg.capi.MODEL_VICTORIAPARK_3D, max_particles=48 * 3)
    host = _vp_run(pkg, sc, make, n, 3, 48, 4, 3.0, 900, device_motion=True, draw_every_update=True)
    dev = _vp_run(pkg, sc, make, n, 3, 48, 4, 3.0, 900, device_cycle=True)
    print("lidar updates %d, resamplings %d (forced %d), largest grown set %d, final count %d" %
          (host.n_lidar, host.n_resamples, host.n_forced, host.n_grown_max, host.n))
    assert host.n_grown_max > n and host.n_forced >= 1
    assert dev.n_lidar == host.n_lidar and dev.n_resamples == host.n_resamples and dev.n == host.n
    ref.assert_same_state(ref.state(host.f), ref.state(dev.f))
    host.f.close(); dev.f.close()
    VP = pkg.capi.MODEL_VICTORIAPARK_3D
    hp = _vp_run(pkg, sc, make, n, 3, 48, 4, 3.0, 900, draw_every_update=True)
    orc = _vp_run(pkg, sc, lambda: ob.OracleFilter(n, model=VP, max_particles=48 * 3), n, 3, 48, 4, 3.0, 900, draw_every_update=True)
    assert hp.n == orc.n and hp.n_lidar == orc.n_lidar and hp.n_resamples == orc.n_resamples >= 1
    assert hp.n_grown_max == orc.n_grown_max > n
    assert np.array_equal(hp.x, orc.x)                         # the host poses followed the same parents and plans
    np.testing.assert_allclose(hp.f.get_weights(), orc.f.get_weights(), rtol=1e-6)
    assert np.array_equal(hp.f.gm_sizes(), orc.f.gm_sizes())
    for i in range(hp.n):
        sc.assert_gm_close(hp.f.export_gm(i), orc.f.export_gm(i), 1e-7, 1e-9)
    hp.f.close()


def _far_candidates(k, dm):
    """k landmark candidates no measurement supports (a kilometre away), young enough never to expire in a test."""
    mean = np.zeros((k, dm))
    mean[:, 0] = 1000.0 + 10.0 * np.arange(k)
    mean[:, 1] = 1000.0
    if dm == 3:
        mean[:, 2] = 0.5
    return mean, np.tile(np.eye(dm) * 0.01, (k, 1, 1)), np.ones(k, np.int32), np.zeros(k, np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("vp", [True, False])
def test_candidate_list_at_its_bound(pkg, sc, vp):
    """One particle.  A probe update from an empty list tells how many candidates this update queues (c); with 64 - c planted
    beforehand the list ends at exactly 64 and the handle stays clean, with 65 - c the 65th is refused at the next synchronising call
    -- on both routes, which also agree on the state left behind."""
    scen = sc.make_vp_scenario(n_particles=1, **VP_KW["const"]) if vp else mh.crowded(sc, 1)
    dm = 3 if vp else 2

    def pair():
        fs = ref.make_pair(pkg, sc, scen, 1, 4, 0, 2)
        for f in fs:
            f.fs_config.landmarkCandidateMeasurementCheckThreshold = 100
            f.set_fastslam_config(f.fs_config)
        return fs

    probe, other = pair()
    other.close()
    probe.predict_map()
    probe.update_and_resample(scen["Z"], u01_fn=lambda: 0.5)
    c = len(probe.export_birth_candidates(0)[2])
    probe.close()
    print("%s: the update queues %d candidates" % ("vp" if vp else "2-D", c))
    assert 1 <= c < 64
    for planted, clean in ((64 - c, True), (65 - c, False)):
        host, dev = pair()
        for f in (host, dev):
            f.import_birth_candidates(0, *_far_candidates(planted, dm))
            f.predict_map()
        if clean:
            for f in (host, dev):
                assert f.update_and_resample(scen["Z"], u01_fn=lambda: 0.5) is False
            assert len(dev.export_birth_candidates(0)[2]) == 64
        else:
            with pytest.raises(pkg.capi.EngineError) as eh:
                host.update_and_resample(scen["Z"], u01_fn=lambda: 0.5)
            dev.cycle_async(scen["Z"], 0.5)                      # enqueued without complaint ...
            with pytest.raises(pkg.capi.EngineError) as ed:
                dev.synchronize()                                # ... reported by the next synchronising call
            assert eh.value.status == ed.value.status == pkg.capi.ERR_UNSUPPORTED
            assert "candidate" in str(ed.value)
            dev.synchronize()                                    # once
            assert len(dev.export_birth_candidates(0)[2]) == 64
        a, b = ref.state(host), ref.state(dev)
        for k in ("sizes", "fov", "unused"):
            assert np.array_equal(a[k], b[k]), k
        for x, y in zip(a["cands"][0], b["cands"][0]):
            assert np.array_equal(x, y)
        for x, y in zip(a["maps"][0], b["maps"][0]):
            assert np.array_equal(x, y)
        host.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n0,hyp,n_init,branch,vp", [(13, 3, 13, "forced", True), (65, 3, 20, "forced", False), (13, 3, 13, "neff", True), (65, 3, 64, "neff", False)])
def test_shrinking_resample_with_candidate_lists(pkg, sc, n0, hyp, n_init, branch, vp):
    """resampleWithMapCopy on a grown set whose particles carry candidate lists: the forced branch (grown count > nParticlesMax) and
    the N_eff branch.  A condition on the inputs, asserted: no sample point lies within 1e-9 of a cumulative sum of the host route's
    normalised weights, and N_eff is 1e-6 (relative) from its threshold -- the margins of test_shrinking_resample."""
    scen = sc.make_vp_scenario(n_particles=n0, n_landmarks=12, n_z=8, seed=112, scan="const") if vp else mh.crowded(sc, n0)
    cap = n0 * hyp + 1
    u01 = 0.37
    rz = np.random.default_rng(3)
    Zw = scen["Z"] + rz.normal(0, 1e-3, scen["Z"].shape)
    eff = (0.0, 0.0)
    if branch == "neff":        # the threshold sits a factor 1.5 above the N_eff of this very update, measured on a probe handle
        probe, other = ref.make_pair(pkg, sc, scen, hyp, 4, 0, cap)
        other.close()
        ref.warm_up((probe,), Zw)
        probe.predict_map()
        probe.update_and_resample(scen["Z"])
        w = probe.get_weights()
        eff = (1.5 / float(np.sum(w * w)), 0.0)
        probe.close()
    host, dev = ref.make_pair(pkg, sc, scen, hyp, 4, 0, cap)      # (threshold 4: two sightings promote nothing, the lists stay populated)
    ref.warm_up((host, dev), Zw)
    seen = []
    for f in (host, dev):
        f.n_init = n_init
        f.effNParticles_t, f.effNParticles_t_percent = eff
        f.fs_config.minUpdatesBeforeResample = 1
        f.fs_config.nParticlesMax = n0 * hyp - 1 if branch == "forced" else cap
        f.predict_map()
    assert host.update_and_resample(scen["Z"], u01_fn=lambda: (seen.append(host.get_weights().copy()), u01)[1]) is True
    grown = seen[0].size
    assert grown == n0 * hyp
    near, neff = mh.resample_margins(seen[0], u01, min(n_init, grown))
    print("%s %s: grown %d -> %d, N_eff %.6g, nearest sample point / cumulative sum %.3g" % ("vp" if vp else "2-D", branch, grown, host.n, neff, near))
    assert near >= 1e-9
    if branch == "neff":
        assert abs(neff / eff[0] - 1) >= 1e-6
    assert dev.update_and_resample(scen["Z"], u01_fn=lambda: u01) is True
    lc = dev.last_cycle
    assert lc["n_after_update"] == grown and lc["fired"] and dev.n == host.n == min(n_init, grown)
    assert np.array_equal(lc["parent"], host.parents)
    assert np.array_equal(lc["plan"], host.last_resample_plan)
    a, b = ref.state(host), ref.state(dev)
    assert sum(len(c[2]) for c in a["cands"]) > 0, "no candidate list travelled"
    ref.assert_same_state(a, b)
    host.close(); dev.close()
