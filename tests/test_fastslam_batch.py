"""A filter batch of 2-D single-hypothesis FastSLAM filters (rfsgpu_batch_set_fastslam_config / rfsgpu_batch_fastslam_cycle_async; csrc/fastslam.h
FsBatchArg): every filter must equal a separate FastSLAM handle given the same inputs -- mixtures bit for bit, resampling decisions and
plans exactly, weights to 1e-12 (the tolerance of tests/test_filter_batch.py: the handle's sums are taken over another tree) -- and the CPU
oracle to the tolerances of tests/test_gpu_parity.py; the device loop and the per-step error serve it as they serve an RB-PHD batch."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import device_loop_reference as dl

NEW_SYMBOLS = {"rfsgpu_batch_set_fastslam_config": 3, "rfsgpu_batch_fastslam_cycle_async": 8}     # name -> C arguments


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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
        assert raw.index("/* ---- [batch]") < raw.index("int " + name + "(") < raw.index("/* ---- [metric]"), name + " is not in the [batch] section"
    core = {w for line in re.findall(r"RFSGPU_CORE:(.*)", open(os.path.join(ROOT, "include", "rfsgpu.h")).read()) for w in line.split()}
    assert not (set(NEW_SYMBOLS) & core)
    assert hasattr(pkg, "FastSLAMBatch") and hasattr(pkg.capi.CBatch, "batch_fastslam_cycle_async_packed")


def test_fastslam_sim_configuration_matches_the_shipped_xml(pkg):
    import xml.etree.ElementTree as ET
    r = ET.parse(os.path.join(ROOT, "tests", "golden", "fastslam2dSim_c1.xml")).getroot()
    P = pkg.sim2d_driver.C1_FASTSLAM_SIM
    g = lambda path: float(r.find(path).text)
    assert P["kmax"] == g("timesteps") and P["dt"] == g("sec_per_timestep")
    assert P["Pd"] == g("measurements/probDetection") and P["clutter"] == g("measurements/clutterIntensity")
    assert P["rmax"] == g("measurements/rangeLimitMax") and P["rmin"] == g("measurements/rangeLimitMin") and P["rbuf"] == g("measurements/rangeLimitBuffer")
    assert P["p_noise_inflation"] == g("filter/predict/processNoiseInflationFactor")
    assert P["z_noise_inflation"] == g("filter/update/measurementNoiseInflationFactor")
    assert P["max_hypotheses"] == g("filter/update/maxNDataAssocHypotheses") and P["max_loglik_diff"] == g("filter/update/maxDataAssocLogLikelihoodDiff")
    assert P["kf_range"] == g("filter/update/KalmanFilter/innovationThreshold/range") and P["kf_bearing"] == g("filter/update/KalmanFilter/innovationThreshold/bearing")
    assert P["min_log_likelihood"] == g("filter/weighting/minLogMeasurementLikelihood")
    assert P["eff_n"] == g("filter/resampling/effNParticle") and P["min_updates"] == g("filter/resampling/minTimesteps")
    assert P["existence_prune_thr"] == g("filter/prune/threshold")


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

PDS = [0.99, 0.5, 0.9, 0.7, 0.95, 0.6]
CLUTTERS = [1e-4, 5e-2, 1e-3, 1e-2, 5e-3, 1e-1]
PRUNE_AT = [0, 4, 0, 3, 5, 1]            # pruningMeasurementsThreshold per filter: some cycles find a filter below and another at / above its own


def _grid(sim, n, K, n_landmarks=None):
    Ps, datas, seeds = [], [], []
    for b in range(n):
        P = dict(sim.C1_FASTSLAM_SIM)
        P["Pd"], P["clutter"], P["pruning_meas_threshold"] = PDS[b % 6], CLUTTERS[b % 6], PRUNE_AT[b % 6]
        Ps.append(P)
        datas.append(sim.generate(P, traj_seed=11 + b, kmax=K))
        seeds.append(500 + b)
    return Ps, datas, seeds


def _lockstep_against_handles(pkg, nF, nP, K, every=10):
    sim = pkg.sim2d_driver
    Ps, datas, seeds = _grid(sim, nF, K)
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
    hs = [pkg.FastSLAM(nP, gm_capacity=256) for _ in range(nF)]
    A = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True)
    H = sim.Sim2dBatchRun(hs, datas, Ps, seeds, fastslam=True)
    empty_scan = mixed_prune = False
    for k in range(1, K):
        fa, fh = A.step(k), H.step(k)
        nz = np.array([len(d["Z"][k]) for d in datas])
        thr = np.array([P["pruning_meas_threshold"] for P in Ps])
        empty_scan |= bool((nz == 0).any())
        mixed_prune |= bool(((nz > 0) & (nz < thr)).any() and ((nz > 0) & (nz >= thr)).any())
        np.testing.assert_array_equal(fa, fh, err_msg=f"step {k}: resampling decisions")
        for b in range(nF):
            np.testing.assert_array_equal(A.last_plans[b], H.last_plans[b], err_msg=f"step {k} filter {b}: plan")
        sizes = batch.gm_sizes()
        w = batch.get_weights()
        for b in range(nF):
            np.testing.assert_array_equal(sizes[batch.block(b)], hs[b].gm_sizes(), err_msg=f"step {k} filter {b}: sizes")
            np.testing.assert_allclose(w[batch.block(b)], hs[b].get_weights(), rtol=1e-12, atol=0, err_msg=f"step {k} filter {b}: weights")
        if k % every == 0 or k == K - 1:
            for b in range(nF):
                for i in range(nP):
                    for x, y in zip(batch.export_gm(b * nP + i), hs[b].export_gm(i)):
                        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"step {k} filter {b} particle {i}")
    batch.synchronize()
    out = dict(resamples=A.n_resamples.copy(), empty_scan=empty_scan, mixed_prune=mixed_prune, max_size=int(batch.gm_sizes().max()))
    batch.close()
    for h in hs:
        h.close()
    return out


@pytest.mark.gpu
def test_batch_of_six_equals_six_handles_bit_for_bit(pkg):
    """6 x 200 particles, distinct Pd / clutter / seeds / pruning thresholds, 300 simulator steps in the host loop."""
    r = _lockstep_against_handles(pkg, 6, 200, 300)
    assert (r["resamples"] >= 1).all(), r["resamples"]
    assert r["empty_scan"], "no filter had an empty scan"
    assert r["mixed_prune"], "no cycle had a filter below and a filter at / above its pruningMeasurementsThreshold"
    assert r["max_size"] > 3


@pytest.mark.gpu
def test_batch_of_one_equals_a_plain_handle(pkg):
    r = _lockstep_against_handles(pkg, 1, 200, 300)
    assert r["resamples"][0] >= 1


WEIGHT_RTOL, GM_RTOL, GM_ATOL = 1e-9, 1e-10, 1e-12       # tests/test_gpu_parity.py: compare_weights / compare_maps


def _compare_block_with_oracle(sc, batch, b, orc, what):
    """_compare_fastslam of tests/test_gpu_parity.py for filter b of a batch (no candidate lists: the count threshold is 1)."""
    nP = batch.n_per_filter
    wd, wo = batch.get_weights()[batch.block(b)], orc.get_weights()
    assert np.all(np.isfinite(wd)), what
    np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=WEIGHT_RTOL, atol=1e-300, err_msg=what)
    np.testing.assert_allclose(wd, wo, rtol=1e-8, atol=0, err_msg=what)
    assert np.array_equal(batch.gm_sizes()[batch.block(b)], orc.gm_sizes()), what
    for i in range(nP):
        sc.assert_gm_close(batch.export_gm(b * nP + i), orc.export_gm(i), GM_RTOL, GM_ATOL, ordered=True)


@pytest.mark.gpu
def test_simulator_loop_against_the_cpu_oracle(pkg, ob, sc):
    sim = pkg.sim2d_driver
    nF, nP, K = 3, 64, 160
    Ps, datas, seeds = _grid(sim, nF, K)
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
    orcs = [ob.OracleFilter(nP) for _ in range(nF)]
    A = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True)
    O = sim.Sim2dBatchRun(orcs, datas, Ps, seeds, fastslam=True)
    for k in range(1, K):
        fa, fo = A.step(k), O.step(k)
        np.testing.assert_array_equal(fa, fo, err_msg=f"step {k}: resampling decisions")
        if k % 10 == 0 or k == K - 1:
            for b in range(nF):
                np.testing.assert_array_equal(A.last_plans[b], O.last_plans[b])
                _compare_block_with_oracle(sc, batch, b, orcs[b], f"step {k} filter {b}")
    assert A.n_resamples.sum() >= 1
    batch.close()


@pytest.mark.gpu
def test_ragged_scenario_in_every_filter_with_different_scans(pkg, ob, sc):
    """FS_SCENARIOS' ragged class (70 landmarks = 64 + 6) in each of four filters, n_z 19 / 0 / 7 / 12, three cycles."""
    from test_filter_batch import _configure_from_scenario
    scen = sc.make_scenario(n_particles=24, n_landmarks=70, n_z=19, seed=62)
    nF, nP = 4, scen["n"]
    nzs = [19, 0, 7, 12]
    logodds = [np.log(scen["w"][i] / (1 - scen["w"][i] * 0.5)) for i in range(nP)]
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
    batch.set_poses(np.vstack([scen["poses"]] * nF), np.vstack([np.tile(np.asarray(scen["pose_cov"], dtype=np.float64).ravel(), (nP, 1))] * nF))
    batch.set_weights(np.concatenate([scen["particle_w"]] * nF))
    orcs = []
    for b in range(nF):
        _configure_from_scenario(pkg.capi, batch, b, scen["params"])
        batch.configure_fastslam(b, batch.default_fastslam_config())
        for i in range(nP):
            batch.import_gm(b * nP + i, logodds[i], scen["mean"][i], scen["cov"][i])
        o = ob.OracleFilter(nP)
        sc.load_scenario(o, scen)
        for i in range(nP):
            o.import_gm(i, logodds[i], scen["mean"][i], scen["cov"][i])
        o.set_fastslam_config(o.default_fastslam_config())
        orcs.append(o)
    rng = np.random.default_rng(62)
    for step in range(3):
        Z = scen["Z"] + rng.normal(0, 2e-3, scen["Z"].shape)
        batch.cycle_async(True, [Z[:n] for n in nzs], normalize=False)
        for b, o in enumerate(orcs):
            o.predict_map(False)
            if nzs[b]:
                o.fastslam_update(Z[:nzs[b]])
            _compare_block_with_oracle(sc, batch, b, o, f"cycle {step} filter {b}")
        batch.cycle_async(None, [np.zeros((0, 2))] * nF, normalize=True)     # nothing moves without measurements, not even the weights
        for b, o in enumerate(orcs):
            _compare_block_with_oracle(sc, batch, b, o, f"cycle {step} filter {b}: after an empty cycle")
        w = batch.get_weights()
        for b, o in enumerate(orcs):
            if nzs[b]:
                s = o.weight_sums()
                o.normalize_weights(s[0])
                blk = batch.block(b)
                w[blk] = w[blk] / w[blk].sum()
        batch.set_weights(w)
    batch.close()


def _sequential_neff(w):
    s = 0.0
    for v in w:
        s += float(v) * float(v)
    return 1.0 / s


@pytest.mark.gpu
def test_device_loop_propagation_and_resampling_rule(pkg):
    """Propagation against tests/support/device_loop_reference.py::propagate (the tolerance of tests/test_batch_device_loop.py: 1e-10, the
    libm calls differ); every resample_async decision, plan and N_eff against the host rule on the weights read back just before; the
    mixtures after a resampling are the gathered ones bit for bit."""
    sim = pkg.sim2d_driver
    nF, nP, K = 4, 200, 300
    Ps, datas, seeds = _grid(sim, nF, K)
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
    run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True, device_loop=True)
    eff_n = np.array([P["eff_n"] for P in Ps])
    cnt_u, cnt_m = np.zeros(nF, dtype=np.int64), np.zeros(nF, dtype=np.int64)
    total = np.zeros(nF, dtype=np.int64)
    checked_gather = 0
    for k in range(1, K):
        x0 = batch.get_poses()
        run._device_propagate(k)
        got = batch.get_poses()
        for b in range(nF):
            blk = batch.block(b)
            want = np.tile(datas[b]["gt"][k], (nP, 1)) if k <= 100 else dl.propagate(x0[blk], datas[b]["odom"][k], np.diag(run.Q[b]), seeds[b], k)
            np.testing.assert_allclose(got[blk], want, rtol=1e-10, atol=1e-10, err_msg=f"step {k} filter {b}: poses")
        nz = run._nz[k]
        batch.batch_fastslam_cycle_async_packed(True, run._z[k], nz, normalize=True)
        w = batch.get_weights()
        # the host rule on the weights read back just now, before the device decides
        want_fire, want_plan, want_neff = np.zeros(nF, dtype=bool), np.arange(batch.n), np.zeros(nF)
        for b in range(nF):
            blk = batch.block(b)
            cnt_u[b] += 1
            if nz[b] > 0:
                cnt_m[b] += nz[b]
                if cnt_u[b] >= Ps[b]["min_updates"] and cnt_m[b] >= 1:
                    ne = _sequential_neff(w[blk])
                    assert abs(ne - eff_n[b]) > 1e-9 * eff_n[b]
                    want_neff[b] = ne
                    want_fire[b] = not (ne > eff_n[b] and ne / nP > eff_n[b] / nP)
                    if want_fire[b]:
                        want_plan[blk] = blk.start + pkg.engine.systematic_resample_plan(w[blk], dl.resample_draw(seeds[b], k))
                        cnt_u[b] = cnt_m[b] = 0
        before = None
        if want_fire.any() and checked_gather < 3:      # every slot of the filters about to resample, as it is before the gather
            before = {i: batch.export_gm(i) for b in np.nonzero(want_fire)[0] for i in range(b * nP, (b + 1) * nP)}
        batch.resample_async(nz, k)
        fired, plan, neff = batch.last_resample()
        np.testing.assert_array_equal(fired, want_fire, err_msg=f"step {k}: decisions")
        np.testing.assert_array_equal(plan, want_plan, err_msg=f"step {k}: plans")
        for b in range(nF):
            if want_neff[b]:
                np.testing.assert_allclose(neff[b], want_neff[b], rtol=1e-14)
        total += fired
        if before is not None:
            assert (plan[list(before)] != np.array(list(before))).any()
            for i in before:
                for x, y in zip(batch.export_gm(i), before[int(plan[i])]):
                    np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"step {k}: slot {i} after the gather")
            for b in np.nonzero(fired)[0]:
                np.testing.assert_array_equal(batch.get_weights()[batch.block(b)], np.ones(nP))
            checked_gather += 1
    np.testing.assert_array_equal(batch.resample_counts(), total)
    assert (total >= 1).all() and checked_gather >= 1
    batch.close()


@pytest.mark.gpu
def test_free_running_device_loop_64_filters(pkg):
    """64 x 200 particles, 100 steps, nothing read back before the end: every filter has resampled, the error word is clear."""
    sim = pkg.sim2d_driver
    nF, nP, K = 64, 200, 101
    Ps, datas, seeds = _grid(sim, nF, K)
    for P in Ps:
        P["eff_n"] = 250.0        # (for k <= 100 the particles are pinned to the ground truth and N_eff stays at 200: a threshold above the
                                  #  particle count resamples whenever the two gates pass, so the gather runs every other step)
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
    run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True, device_loop=True)
    run.run(1, K)
    batch.synchronize()            # raises if the shared error word is set
    assert (run.resample_counts() > 0).all(), run.resample_counts()
    assert batch.gm_sizes().max() > 0 and np.all(np.isfinite(batch.get_weights()))
    batch.close()


def _tool():
    spec = importlib.util.spec_from_file_location("analysis2d_sim", os.path.join(ROOT, "tools", "analysis2d_sim.py"))
    a = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(a)
    return a


@pytest.mark.gpu
def test_step_error_on_a_fastslam_batch(pkg):
    """Planted maps whose log-odds lie on both sides of the threshold (every transformed weight >= 1e-6 away from it): the record agrees
    with tools/analysis2d_sim.py fed 1 - 1 / (1 + exp(w)) at 1e-12 (tests/test_step_error.py's tolerance); an ordinary FastSLAM handle
    still refuses."""
    import test_step_error as tse
    a = _tool()
    nF, nP = 3, 8
    rng = np.random.default_rng(77)
    thr, c, p = 0.75, 0.20, 1.0
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=64)
    sim = pkg.sim2d_driver
    for b in range(nF):
        sim.configure_fastslam_batch_filter(batch, b)
    wp = rng.uniform(0.05, 1.0, nF * nP)
    batch.set_weights(wp)
    x = rng.normal(0, 0.2, (nF * nP, 3))
    batch.set_poses(x)
    truths, planted = [], {}
    for b in range(nF):
        truth = rng.uniform(-3, 3, (9 + b, 2))
        truths.append(truth)
        batch.set_ground_truth(truth, None, filter=b)
        for i in range(nP):
            m = 6 + (i + b) % 5
            pr = rng.uniform(0.05, 0.98, m)
            pr[np.abs(pr - thr) < 1e-3] = 0.9          # (no transformed weight within 1e-6 of the threshold)
            lo = np.log(pr / (1 - pr))
            mean = truth[rng.integers(0, len(truth), m)] + rng.normal(0, 0.03, (m, 2))
            batch.import_gm(b * nP + i, lo, mean, np.tile(np.eye(2) * 0.01, (m, 1, 1)))
            planted[b * nP + i] = (lo, mean)
    # (rfsgpu_batch_set_fastslam_config has made this a FastSLAM batch: the maps are read as log-odds before any cycle has run)
    gt_pose = rng.normal(0, 0.1, (nF, 3))
    rows = batch.step_error(np.zeros(nF), gt_pose, thr, c, p)
    both_sides = 0
    for b in range(nF):
        blk = batch.block(b)

        class View:      # the batch with log-odds turned into the logged existence probability: what analysis2dSim reads
            def get_weights(self):
                return batch.get_weights()

            def get_poses(self):
                return batch.get_poses()

            def export_gm(self, slot):
                w, wp_, mean, cov = batch.export_gm(slot)
                return 1 - 1 / (1 + np.exp(w)), wp_, mean, cov
        want = tse._host_row(a, View(), blk, truths[b], np.full(len(truths[b]), -1.0), 0.0, gt_pose[b], thr, c, p)
        pr = 1 - 1 / (1 + np.exp(planted[int(want["best_slot"])][0]))
        assert np.abs(pr - thr).min() >= 1e-6
        both_sides += int((pr >= thr).any() and (pr < thr).any())
        tse._check_row(rows[b], want, f"filter {b}")
        mean, cov, w = batch.get_map_estimate(thr, filter=b)
        assert len(w) == want["n_est"] and (w >= thr).all()
        np.testing.assert_allclose(np.sort(w), np.sort(pr[pr >= thr]), rtol=1e-13)
    assert both_sides == nF
    batch.close()
    h = pkg.FastSLAM(8, gm_capacity=32)
    sim.configure_fastslam(h)
    h.set_poses(np.zeros((8, 3)))
    h.fastslam_update(np.array([[1.0, 0.1]]))
    with pytest.raises(pkg.capi.EngineError) as e:
        h.set_ground_truth(truths[0])
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED and "FastSLAM handle" in str(e.value)
    h.close()


@pytest.mark.gpu
def test_tracked_and_untracked_runs_end_with_the_same_bits(pkg):
    sim = pkg.sim2d_driver
    nF, nP, K = 4, 100, 150
    Ps, datas, seeds = _grid(sim, nF, K)
    ends = []
    for track in (False, True):
        batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=256)
        run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True, device_loop=True, track_errors=track)
        run.run(1, K)
        if track:
            log = run.errors()
            assert log.shape == (K - 1, nF) and (log["status"] == 0).all()
            assert np.isfinite(log["cola"]).all() and (log["n_truth"][-1] > 0).all() and (log["n_est"][-1] > 0).any()
        batch.synchronize()
        ends.append((batch.get_weights(), batch.get_poses(), batch.gm_sizes(), [batch.export_gm(i) for i in range(0, batch.n, 5)]))
        batch.close()
    np.testing.assert_array_equal(_bits(ends[0][0]), _bits(ends[1][0]))
    np.testing.assert_array_equal(_bits(ends[0][1]), _bits(ends[1][1]))
    np.testing.assert_array_equal(ends[0][2], ends[1][2])
    for g0, g1 in zip(ends[0][3], ends[1][3]):
        for x, y in zip(g0, g1):
            np.testing.assert_array_equal(_bits(x), _bits(y))


@pytest.mark.gpu
def test_refusals(pkg):
    capi = pkg.capi
    batch = pkg.FastSLAMBatch(2, 16, gm_capacity=32)
    cfg = batch.default_fastslam_config()
    cfg.maxNDataAssocHypotheses = 2
    with pytest.raises(capi.EngineError) as e:
        batch.configure_fastslam(1, cfg)
    assert e.value.status == capi.ERR_UNSUPPORTED and "filter 1" in str(e.value) and "maxNDataAssocHypotheses" in str(e.value)
    cfg = batch.default_fastslam_config()
    cfg.landmarkCandidateMeasurementCountThreshold = 2
    with pytest.raises(capi.EngineError) as e:
        batch.configure_fastslam(0, cfg)
    assert e.value.status == capi.ERR_UNSUPPORTED and "filter 0" in str(e.value) and "landmarkCandidateMeasurementCountThreshold" in str(e.value)
    none = [np.zeros((0, 2))] * 2
    batch.cycle_async(True, none)
    with pytest.raises(capi.EngineError) as e:
        batch.batch_cycle_async(True, none)
    assert e.value.status == capi.ERR_UNSUPPORTED and "FastSLAM" in str(e.value) and "one kind" in str(e.value)
    with pytest.raises(capi.EngineError) as e:                      # the single handle's call stays refused on a batch
        batch.fastslam_update(np.array([[1.0, 0.0]]))
    assert e.value.status == capi.ERR_UNSUPPORTED
    batch.close()
    other = pkg.FilterBatch(2, 16, gm_capacity=32)
    other.cycle_async(True, none)
    with pytest.raises(capi.EngineError) as e:
        other.batch_fastslam_cycle_async(True, none)
    assert e.value.status == capi.ERR_UNSUPPORTED and "RB-PHD" in str(e.value) and "one kind" in str(e.value)
    with pytest.raises(capi.EngineError) as e:
        other.batch_set_fastslam_config(None, other.default_fastslam_config())
    assert e.value.status == capi.ERR_UNSUPPORTED and "one kind" in str(e.value)
    other.close()
    third = pkg.FastSLAMBatch(2, 16, gm_capacity=32)             # the configuration call alone fixes the kind
    third.configure_fastslam(None, third.default_fastslam_config())
    with pytest.raises(capi.EngineError) as e:
        third.batch_cycle_async(True, none)
    assert e.value.status == capi.ERR_UNSUPPORTED and "one kind" in str(e.value)
    third.close()
    with pytest.raises(capi.EngineError) as e:
        capi.CBatch(pkg.load_library(), "rfsgpu_", 2, 16, model=capi.MODEL_VICTORIAPARK_3D)
    assert e.value.status == capi.ERR_UNSUPPORTED and "Victoria Park" in str(e.value)


@pytest.mark.gpu
def test_capacity_overflow_names_the_lowest_filter(pkg):
    """Filters 1 and 2 of four stand at gm_capacity with landmarks out of range; one measurement nothing takes asks for a new landmark:
    the shared error word is raised at the next synchronising call and rfsgpu_last_error names filter 1."""
    sim = pkg.sim2d_driver
    nF, nP, cap = 4, 8, 64
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=cap)
    for b in range(nF):
        sim.configure_fastslam_batch_filter(batch, b)
    batch.set_poses(np.zeros((nF * nP, 3)))
    far = np.column_stack([np.linspace(50, 80, cap), np.full(cap, 40.0)])
    for b in (1, 2):
        for i in range(nP):
            batch.import_gm(b * nP + i, np.full(cap, 2.0), far, np.tile(np.eye(2) * 0.01, (cap, 1, 1)))
    Z = np.array([[1.5, 0.3]])
    batch.cycle_async(True, [Z] * nF, normalize=True)
    with pytest.raises(pkg.capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "gm_capacity exceeded in filter 1" in str(e.value), str(e.value)
    sizes = batch.gm_sizes().reshape(nF, nP)
    assert (sizes[0] == 1).all() and (sizes[3] == 1).all() and (sizes[1] == cap).all() and (sizes[2] == cap).all()
    batch.cycle_async(True, [Z, np.zeros((0, 2)), np.zeros((0, 2)), Z], normalize=True)       # the word was cleared: the batch goes on
    batch.synchronize()
    batch.close()


@pytest.mark.gpu
def test_one_wave_fall_back_of_the_associate_kernel(pkg):
    """At gm_capacity 576 two waves' LDS exceeds 64 KB and the associate kernel runs one wave per workgroup, for a handle
    (fs_associate_update_kernel<1, 2>) and for a batch (fs_associate_update_batch_kernel<1>): three filters x 33 particles (an odd count:
    the filters' blocks do not align with anything) against their handles over 130 steps, mixtures bit for bit."""
    sim = pkg.sim2d_driver
    nF, nP, K, cap = 3, 33, 130, 576
    Ps, datas, seeds = _grid(sim, nF, K)
    batch = pkg.FastSLAMBatch(nF, nP, gm_capacity=cap)
    hs = [pkg.FastSLAM(nP, gm_capacity=cap) for _ in range(nF)]
    A = sim.Sim2dBatchRun(batch, datas, Ps, seeds, fastslam=True)
    H = sim.Sim2dBatchRun(hs, datas, Ps, seeds, fastslam=True)
    for k in range(1, K):
        np.testing.assert_array_equal(A.step(k), H.step(k), err_msg=f"step {k}: decisions")
        if k % 10 == 0 or k == K - 1:
            for b in range(nF):
                np.testing.assert_array_equal(A.last_plans[b], H.last_plans[b])
                np.testing.assert_allclose(batch.get_weights()[batch.block(b)], hs[b].get_weights(), rtol=1e-12, atol=0)
                for i in range(nP):
                    for x, y in zip(batch.export_gm(b * nP + i), hs[b].export_gm(i)):
                        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"step {k} filter {b} particle {i}")
    assert batch.gm_sizes().max() > 3 and A.n_resamples.sum() >= 1
    batch.close()
