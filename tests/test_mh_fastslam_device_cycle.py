"""rfsgpu_fastslam_cycle_async: one whole multi-hypothesis FastSLAM::update on the device -- the copy plan (fs_mh_plan_kernel), the
count-guarded launches of the update, and resampleWithMapCopy (fs_resample_shrink_kernel) -- without a host stop.

The yardstick is the host-planned route on a second handle given the same state, the same measurements and the same draw:
rfsgpu_fastslam_update + engine.FastSLAM.update_and_resample (device_cycle=False).  The same kernels run on the same inputs on
both routes, in the same order -- the weight sum and the normalisation included -- so states are compared bit for bit; the
normalised weights as well, which is stricter than the 1e-12 two differently ordered sums would need.

What is not compared: the raw (un-normalised) weights of the device route.  A cycle ends with its normalisation or its resampling,
and no call shows the weights in between; the normalised ones are held bit-equal instead.  A particle without any hypothesis
(nH == 0) arises on the device only when its table is refused (more than 64 rows): the host route then stops before it plans
anything while the device route's other particles go on, so the two states are not comparable and that sub-case is left to the
CPU test of the plan.

The resampling decisions: before plans are compared the test asserts, on the host route's own normalised weights, that every sample
point is at least 1e-9 from every cumulative sum and N_eff at least 1e-6 (relative) from its thresholds, so no rounding in the last
place decides anything.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import mh_device_cycle_reference as ref


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_new_calls_are_exported_with_the_header_s_arguments(pkg):
    pkg.build_mod.build()
    lib = pkg.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfsgpu.h")).read(), flags=re.S)
    want = {
        "rfsgpu_fastslam_cycle_async": "rfsgpu_filter *f, int predict, const double *z, int n_z, double u01, int n_init",
        "rfsgpu_fastslam_last_cycle": "rfsgpu_filter *f, int *n_after_update, int *n_after_resample, int *fired, double *n_eff, int *parent, int *plan, int max_n",
        "rfsgpu_fastslam_set_resampling": "rfsgpu_filter *f, double eff_n, double eff_n_percent",
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name + " is not declared"
        assert " ".join(m.group(1).split()) == args
        assert name[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    assert "#define RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES 2048" in txt
    # a null handle is refused before anything else
    lib.rfsgpu_fastslam_cycle_async.restype = C.c_int
    assert lib.rfsgpu_fastslam_cycle_async(C.c_void_p(), C.c_int(0), C.c_void_p(), C.c_int(0), C.c_double(0.5), C.c_int(1)) == pkg.capi.ERR_INVALID


@pytest.mark.parametrize("n0", [1, 63, 64, 65, 255, 256, 257, 300])
def test_copy_plan_scan_form_equals_the_host_loop(n0):
    rng = np.random.default_rng(n0)
    vectors = [rng.integers(0, 2, n0), np.full(n0, 16), np.ones(n0, int), np.zeros(n0, int), rng.integers(0, 17, n0), rng.integers(1, 5, n0)]
    v = rng.integers(1, 17, n0)
    v[rng.integers(0, n0, max(1, n0 // 7))] = 0           # particles without any hypothesis among multiplied ones
    vectors.append(v)
    for nH in vectors:
        got, want = ref.scan_plan(nH), ref.host_loop_plan(nH)
        assert got[0] == want[0] == n0 + int(np.maximum(np.asarray(nH) - 1, 0).sum())
        for g, w, what in zip(got[1:], want[1:], ("slotSrc", "slotHyp", "slotNH", "copyDst", "copySrc")):
            assert np.array_equal(g, w), what
        n, src, hyp, cnt, dst, csrc = got
        assert np.array_equal(np.bincount(src, minlength=n0)[:n0], np.maximum(np.asarray(nH), 1))
        assert sorted(dst.tolist()) == list(range(n0, n)) and np.array_equal(src[dst], csrc)


def test_shrink_plan_margin_helper():
    w = np.array([0.1, 0.2, 0.3, 0.4])
    near, neff = ref.resample_margins(w, 0.5, 2)            # sample points 0.25, 0.75 against 0.1, 0.3, 0.6, 1.0
    assert np.isclose(near, 0.05) and np.isclose(neff, 1 / 0.3)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

NEVER = 1000          # minUpdatesBeforeResample that no test reaches


def _pair(pkg, sc, scen, hyp, diff, cap=None):
    """Two FastSLAM objects with the same state: the host-planned route and the device cycle."""
    n0 = scen["n"]
    out = []
    for dc in (False, True):
        f = pkg.FastSLAM(n0, gm_capacity=64, max_hypotheses=max(hyp, 2), n_particles_max=(cap // max(hyp, 2) if cap else n0), device_cycle=dc)
        ref.load(f, sc, scen, hyp, diff)
        out.append(f)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n0,hyp,kind", [(1, 16, "full"), (63, 4, "full"), (64, 2, "full"), (65, 16, "full"), (257, 4, "full"),
                                         (64, 4, "none"), (65, 4, "window"), (65, 16, "mixed")])
def test_plan_and_update_without_resampling(pkg, sc, n0, hyp, kind):
    """Gates shut: parents, grown count, ordered mixtures, sizes, FOV counts, unused masks and normalised weights equal the
    host-planned route bit for bit.  full: every particle reaches the limit; none: no particle multiplies; window / mixed: the
    likelihood window decides, hypothesis counts differ between particles (1 or 2; 2, 4 or 6)."""
    scen = {"none": ref.sparse, "full": ref.crowded, "window": ref.windowed, "mixed": ref.mixed}[kind](sc, n0)
    diff = {"window": 1.0, "mixed": 8.0}.get(kind, 50.0)
    host, dev = _pair(pkg, sc, scen, hyp, diff)
    assert dev.max_particles == n0 * hyp
    for f in (host, dev):
        f.fs_config.minUpdatesBeforeResample = NEVER
        f.fs_config.nParticlesMax = f.max_particles
        f.predict_map()
        assert f.update_and_resample(scen["Z"], u01_fn=lambda: 0.25) is False
    lc = dev.last_cycle
    print("n0 %d hyp %d %s: grown %d" % (n0, hyp, kind, host.n))
    assert lc["n_after_update"] == lc["n_after_resample"] == host.n == dev.n and not lc["fired"]
    if kind == "full":
        assert host.n == n0 * hyp
    elif kind == "none":
        assert host.n == n0
    else:
        assert n0 < host.n < n0 * hyp
        assert len(set(np.bincount(host.parents, minlength=n0)[:n0].tolist())) >= 2
    assert np.array_equal(lc["parent"], host.parents) and np.array_equal(dev.parents, host.parents)
    assert np.array_equal(lc["plan"], np.arange(host.n))
    a, b = ref.state(host), ref.state(dev)
    np.testing.assert_allclose(b["w"], a["w"], rtol=1e-12, atol=0)
    ref.assert_same_state(a, b)
    host.close(); dev.close()


@pytest.mark.gpu
def test_capacity_exact_fit_passes_and_one_more_copy_is_refused(pkg, sc):
    n0, hyp = 4, 4
    scen = ref.crowded(sc, n0)
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
        dev.set_fastslam_config(cfg)
        before = ref.state(dev)
        dev.fastslam_cycle_async(scen["Z"], 0.5, n0)
        dev.fastslam_cycle_async(scen["Z"], 0.5, n0) if not fits else None      # a cycle enqueued behind the refused one is abandoned with it
        if fits:
            dev.synchronize()
            assert dev.n == 16 and dev.fastslam_last_cycle()["n_after_update"] == 16
        else:
            with pytest.raises(pkg.capi.EngineError) as e:
                dev.synchronize()
            assert e.value.status == pkg.capi.ERR_CAPACITY and "max_particles" in str(e.value)
            dev.synchronize()                                                       # reported once
            ref.assert_same_state(before, ref.state(dev))
            # ... and the handle goes on: the ordinary route refuses the same update for the same reason
            with pytest.raises(pkg.capi.EngineError) as e2:
                dev.fastslam_update(scen["Z"])
            assert e2.value.status == pkg.capi.ERR_CAPACITY
            ref.assert_same_state(before, ref.state(dev))
        dev.close()


# (particles, hypotheses each -> grown count, n_init, which branch).  forced: the grown count exceeds nParticlesMax; neff / percent:
# the gated branch fires on the first / on the second threshold; quiet: the gated branch runs its test and does not fire.
SHRINK = [(1, 2, 1, "forced"), (13, 5, 64, "forced"), (75, 4, 200, "forced"), (128, 16, 64, "forced"), (128, 16, 200, "forced"), (13, 5, 1, "forced"),
          (13, 5, 64, "neff"), (75, 4, 200, "percent"), (13, 5, 64, "quiet"), (75, 4, 200, "quiet")]


@pytest.mark.gpu
@pytest.mark.parametrize("n0,hyp,n_init,branch", SHRINK)
def test_shrinking_resample(pkg, sc, n0, hyp, n_init, branch):
    grown = n0 * hyp
    scen = ref.crowded(sc, n0)
    u01 = 0.37
    eff = (0.0, 0.0)
    if branch != "forced":      # the thresholds sit a factor 1.5 from the N_eff of this very update, measured on a probe handle
        probe = _pair(pkg, sc, scen, hyp, 50.0)[0]
        probe.fs_config.minUpdatesBeforeResample = NEVER
        probe.fs_config.nParticlesMax = grown
        probe.predict_map()
        probe.update_and_resample(scen["Z"])
        w = probe.get_weights()
        neff0 = 1.0 / float(np.sum(w * w))
        probe.close()
        eff = {"neff": (1.5 * neff0, 0.0), "percent": (0.0, 1.5 * neff0 / grown), "quiet": (neff0 / 1.5, neff0 / 1.5 / grown)}[branch]
    host, dev = _pair(pkg, sc, scen, hyp, 50.0)
    seen = []
    for f in (host, dev):
        f.n_init = n_init
        f.effNParticles_t, f.effNParticles_t_percent = eff
        f.fs_config.nParticlesMax = grown - 1 if branch == "forced" else grown
        f.predict_map()
    did = host.update_and_resample(scen["Z"], u01_fn=lambda: (seen.append(host.get_weights().copy()), u01)[1])
    assert did == (branch != "quiet")
    # the margins, on the host route's own normalised weights
    wn = seen[0] if did else host.get_weights()
    assert wn.size == grown
    near, neff = ref.resample_margins(wn, u01, min(n_init, grown))
    print("%s: grown %d -> %d, N_eff %.6g, nearest sample point / cumulative sum %.3g" % (branch, grown, n_init, neff, near))
    if did:
        assert near >= 1e-9
    if branch != "forced":
        for t, v in ((eff[0], neff), (eff[1], neff / grown)):
            assert t == 0.0 or abs(v / t - 1) >= 1e-6
    assert dev.update_and_resample(scen["Z"], u01_fn=lambda: u01) == did
    lc = dev.last_cycle
    assert lc["n_after_update"] == grown and lc["fired"] == did
    assert np.array_equal(lc["parent"], host.parents)
    if branch != "forced":
        assert abs(lc["n_eff"] / neff - 1) < 1e-12        # the sequential sum against numpy's pairwise one
    if did:
        assert dev.n == host.n == lc["n_after_resample"] == min(n_init, grown)
        assert np.array_equal(lc["plan"], host.last_resample_plan) and np.array_equal(dev.last_resample_plan, host.last_resample_plan)
    else:
        assert dev.n == host.n == grown and dev.last_resample_plan is None
    assert np.array_equal(np.array(dev.get_particle_ids()), np.array(host.get_particle_ids()))
    a, b = ref.state(host), ref.state(dev)
    # after a resampling every weight is 1; a quiet test leaves the twice-normalised weights, from the same two kernels twice
    ref.assert_same_state(a, b)
    # the flag carries over: the next update on both routes (its copies inherit under the same rule), gates shut
    for f in (host, dev):
        f.fs_config.minUpdatesBeforeResample = NEVER
        f.fs_config.nParticlesMax = f.max_particles
    if host.n * hyp <= host.max_particles:
        for f in (host, dev):
            f.predict_map()
            f.update_and_resample(scen["Z"], u01_fn=lambda: 0.5)
        assert host.n == dev.n
        ref.assert_same_state(ref.state(host), ref.state(dev))
    host.close(); dev.close()


def _sim_config():
    import xml.etree.ElementTree as ET
    from importlib import import_module
    t = ET.parse(os.path.join(ROOT, "tests", "golden", "mhfastslam2dSim_c1.xml")).getroot()
    return dict(max_hypotheses=int(t.find("filter/update/maxNDataAssocHypotheses").text),
                max_loglik_diff=float(t.find("filter/update/maxDataAssocLogLikelihoodDiff").text),
                min_log_likelihood=float(t.find("filter/weighting/minLogMeasurementLikelihood").text),
                existence_prune_thr=float(t.find("filter/prune/threshold").text),
                eff_n=float(t.find("filter/resampling/effNParticle").text), min_updates=int(t.find("filter/resampling/minTimesteps").text))


@pytest.mark.gpu
def test_thirty_steps_of_the_mh_simulator_configuration(pkg, sc):
    """The filter configuration of tests/golden/mhfastslam2dSim_c1.xml at 50 particles, steps 1 ... 30 (the poses are the ground truth,
    as the driver sets them for the first 100 steps): per-step counts, decisions, parents and plans are equal, and so are the final maps."""
    drv = pkg.sim2d_driver
    # (kmax spaces the generator's landmarks: 3000 would put a single landmark into 30 steps, 120 puts 16 there, a dozen in range)
    P = dict(drv.C1_FASTSLAM_SIM, **_sim_config(), kmax=120)
    assert P["max_hypotheses"] == 3
    data = drv.generate(P, traj_seed=3, kmax=31)
    n0 = 50
    draws = np.random.default_rng(8).random(31)
    fs = []
    for dc in (False, True):
        f = pkg.FastSLAM(n0, gm_capacity=64, max_hypotheses=P["max_hypotheses"], device_cycle=dc)
        drv.configure(f, P)
        f.config = f.get_filter_config()
        f.fs_config = drv.fastslam_config(f, P)
        f.fs_config.nParticlesMax = 3 * n0
        f.setEffectiveParticleCountThreshold(P["eff_n"])
        fs.append(f)
    host, dev = fs
    fired = grew = 0
    for k in range(1, 31):
        Z = data["Z"][k]
        res = []
        for f in fs:
            f.set_poses(np.tile(data["gt"][k], (f.n, 1)), np.zeros((3, 3)))
            f.predict_map()
            res.append(f.update_and_resample(Z, u01_fn=lambda: float(draws[k])))
        assert res[0] == res[1], k
        if len(Z) == 0:
            continue
        lc = dev.last_cycle
        assert host.n == dev.n == lc["n_after_resample"], k
        assert np.array_equal(host.parents, dev.parents), k
        grew += int(lc["n_after_update"] > n0)
        if res[0]:
            fired += 1
            assert np.array_equal(host.last_resample_plan, dev.last_resample_plan), k
        assert (host.nUpdatesSinceResample, host.nMeasurementsSinceResample) == (dev.nUpdatesSinceResample, dev.nMeasurementsSinceResample)
    # What the configuration itself makes of 30 steps, by its own rules: effNParticle (100) is above the 50 particles, so
    # `N_eff / n > 100 / 50` never holds and every cycle whose gates are open resamples -- minTimesteps is 2, every second step.  At
    # step 1 no particle has a landmark: the table is all floor, every assignment ties and every particle reaches its 3 hypotheses.
    # Later growth depends on the realisation (an all-visible static scene resolves most tables to one hypothesis).
    print("resamplings %d, steps whose update multiplied particles %d" % (fired, grew))
    assert fired == 15 and grew >= 1
    a, b = ref.state(host), ref.state(dev)
    np.testing.assert_allclose(b["w"], a["w"], rtol=1e-9, atol=0)            # (tests/test_gpu_parity.py compare_weights)
    for i in range(a["n"]):
        sc.assert_gm_close(a["maps"][i], b["maps"][i], ordered=True)
    ref.assert_same_state(a, b)                                              # ... and in fact bit for bit
    host.close(); dev.close()


@pytest.mark.gpu
def test_five_cycles_enqueued_back_to_back(pkg, sc):
    """No call between the five cycle_async reads or waits: the count, resampleOccured_, the counters and the ids stay on the device.
    The host route, stepped five times with the same measurements and draws, ends in the same state."""
    n0, hyp = 8, 2
    scen = ref.crowded(sc, n0)
    host, dev = _pair(pkg, sc, scen, hyp, 50.0, cap=32)                        # nParticlesMax 16: 8 -> 16 stays, 16 -> 32 is forced back to 8
    assert host.fs_config.nParticlesMax == 16 and dev.max_particles == 32
    rz = np.random.default_rng(4)
    Zs = [scen["Z"] + rz.normal(0, 3e-3, scen["Z"].shape) for _ in range(5)]
    Zs[3] = np.zeros((0, 2))                                                  # an empty scan in the middle: counted, nothing else
    draws = [0.11, 0.52, 0.93, 0.34, 0.75]
    for f in (host, dev):
        f.fs_config.minUpdatesBeforeResample = 2
    for Z, u in zip(Zs, draws):
        dev.cycle_async(Z, u, predict=True)
    counts = []
    for Z, u in zip(Zs, draws):
        host.predict_map()
        host.update_and_resample(Z, u01_fn=lambda: u)
        counts.append(host.n)
    lc = dev.sync_cycle()
    print("host counts per cycle", counts)
    assert counts == [16, 8, 16, 16, 8]
    assert dev.n == host.n == lc["n_after_resample"]
    assert lc["fired"] == host.resampleOccured
    assert np.array_equal(lc["parent"], host.parents)
    if lc["fired"]:
        assert np.array_equal(lc["plan"], host.last_resample_plan)
    assert np.array_equal(np.array(dev.get_particle_ids()), np.array(host.get_particle_ids()))
    ref.assert_same_state(ref.state(host), ref.state(dev))
    host.close(); dev.close()


@pytest.mark.gpu
def test_refused_configurations_leave_the_state_untouched(pkg, sc):
    U = pkg.capi.ERR_UNSUPPORTED
    Z = np.array([[1.0, 0.1], [1.5, -0.4]])

    def refused(f, word, n_z=2):
        n, w = f.n, f.get_weights().copy()
        with pytest.raises(pkg.capi.EngineError) as e:
            f._call("fastslam_cycle_async", C.c_int(0), f._ptr(np.ascontiguousarray(Z[:n_z])), C.c_int(n_z), C.c_double(0.5), C.c_int(4))
        assert e.value.status == U and word in str(e.value), str(e.value)
        assert f.n == n and np.array_equal(f.get_weights(), w)

    batch = pkg.FilterBatch(2, 4, gm_capacity=64)
    refused(batch, "filter batch")
    batch.close()
    group = pkg.FilterGroup(8, [0], gm_capacity=64)
    refused(group.shards[0], "rfsgpu_group")
    group.close()
    vp = pkg.RBPHDFilter(4, gm_capacity=64, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    refused(vp, "Victoria Park")
    vp.close()
    big = pkg.RBPHDFilter(4, gm_capacity=64, max_particles=2049)
    refused(big, "2048")
    big.close()
    f = pkg.RBPHDFilter(4, gm_capacity=64, max_particles=64)
    scen = ref.crowded(sc, 4)
    sc.load_scenario(f, scen)
    before = ref.state(f)
    cfg = f.default_fastslam_config()
    for field, value, word in (("landmarkCandidateMeasurementCountThreshold", 2, "landmarkCandidateMeasurementCountThreshold"),
                               ("maxNDataAssocHypotheses", 0, "[1, 16]"), ("maxNDataAssocHypotheses", 17, "[1, 16]")):
        c2 = f.default_fastslam_config()
        setattr(c2, field, value)
        f.set_fastslam_config(c2)
        refused(f, word)
        ref.assert_same_state(before, ref.state(f))
    # one hypothesis is served: the same pipeline with kmax = 1, equal to the single-hypothesis update's particle count
    f.set_fastslam_config(cfg)
    f.fastslam_cycle_async(scen["Z"], 0.5, 4)
    assert f.n == 4 and np.array_equal(f.fastslam_last_cycle()["parent"], np.arange(4))
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hyp", [1, 4])
def test_ordinary_update_on_a_handle_that_never_cycled(pkg, ob, sc, hyp):
    """rfsgpu_fastslam_update, whose kernels gained an optional argument, against the oracle as test_multi_hypothesis_fastslam holds
    it: counts, parents, weights, maps and candidate lists over two updates with a resampling between them."""
    from tests.test_gpu_parity import _compare_fastslam
    scen = sc.make_scenario(n_particles=10, n_landmarks=25, n_z=10, seed=7, rmax=6.0)
    n0 = scen["n"]
    dev = pkg.RBPHDFilter(n0, gm_capacity=128, max_particles=n0 * hyp * 4)
    orc = ob.OracleFilter(n0)
    for f in (dev, orc):
        sc.load_scenario(f, scen)
        for i in range(n0):
            f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
        cfg = f.default_fastslam_config()
        cfg.maxNDataAssocHypotheses = hyp
        cfg.maxDataAssocLogLikelihoodDiff = 3.0
        cfg.landmarkCandidateMeasurementCountThreshold = 2
        cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
        cfg.landmarkCandidateMeasurementCheckThreshold = 3
        f.set_fastslam_config(cfg)
    rz = np.random.default_rng(12)
    poses = scen["poses"].copy()
    for step in range(2):
        Z = scen["Z"] + rz.normal(0, 3e-3, scen["Z"].shape)
        for f in (dev, orc):
            f.predict_map(False)
            f.fastslam_update(Z)
        assert dev.n == orc.n and (hyp == 1) == (dev.n == n0)
        par = dev.particle_parents()
        assert np.array_equal(par, orc.particle_parents())
        poses = poses[par]
        _compare_fastslam(sc, dev, orc, dev.n)
        for f in (dev, orc):
            f.normalize_weights(f.weight_sums()[0])
        plan = pkg.engine.systematic_resample_plan(orc.get_weights(), 0.41, n_out=n0)
        for f in (dev, orc):
            f.resample_apply(plan, n_out=n0)
            f.fastslam_set_resample_occured(True)
        poses = poses[plan]
        for f in (dev, orc):
            f.set_poses(poses, scen["pose_cov"])
        _compare_fastslam(sc, dev, orc, n0)
    dev.close()
