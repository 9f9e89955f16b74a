"""rfsgpu_create_batch_mh / rfsgpu_batch_fastslam_mh_cycle_async: many 2-D multi-hypothesis FastSLAM filters, each with its own live
particle count on the device, stepped by one launch chain per cycle.

The yardstick is exact: the same filters as separate handles on rfsgpu_fastslam_cycle_async (pkg.FastSLAM(device_cycle=True)), each
created with max_particles = max_per_filter and given the same state, measurements, poses and draws.  Mixtures in order, sizes, FOV
counts, unused masks, parents, plans, ids, counts and decisions are compared bit for bit; normalised weights and N_eff to 1e-12
relative (the bound the batch tests use for differently ordered sums; the batch in fact sums in the handle's order).

Before a plan or a decision is compared the test asserts, on a handle's own normalised weights (a probe handle given the same update
with its gates shut: the same kernels on the same inputs), that every sample point is at least 1e-9 from every cumulative sum and
N_eff at least 1e-6 (relative) from its thresholds, so no rounding decides anything.  In the two multi-cycle tests the probe starts
from the handle's state before the cycle (Rig.snapshot / Rig.assert_margins).  Every test asserts the coverage it claims.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import device_loop_reference as dl
from tests.support import mh_batch_reference as mb
from tests.support import mh_device_cycle_reference as ref

NEVER = mb.NEVER
NEW = {
    "rfsgpu_create_batch_mh": "rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity",
    "rfsgpu_batch_fastslam_mh_cycle_async": "rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, const double *u01",
    "rfsgpu_batch_fastslam_last_cycle": "rfsgpu_filter *f, int *n_after_update, int *n_after_resample, unsigned char *fired, double *n_eff, unsigned char *overflowed, int *parent, int *plan",
    "rfsgpu_batch_live_counts": "rfsgpu_filter *f, int *out",
}


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_new_calls_are_exported_with_the_header_s_arguments(pkg):
    pkg.build_mod.build()
    lib = pkg.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfsgpu.h")).read(), flags=re.S)
    for name, args in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name + " is not declared"
        assert " ".join(m.group(1).split()) == args
        assert name[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    assert hasattr(pkg, "MHFastSLAMBatch")
    for meth in ("configure_fastslam", "cycle_async", "last_cycle", "live_counts"):
        assert hasattr(pkg.MHFastSLAMBatch, meth)
    # a null handle is refused before anything else
    I = pkg.capi.ERR_INVALID
    null = C.c_void_p()
    for name in ("rfsgpu_batch_fastslam_mh_cycle_async", "rfsgpu_batch_fastslam_last_cycle", "rfsgpu_batch_live_counts"):
        getattr(lib, name).restype = C.c_int
    assert lib.rfsgpu_batch_fastslam_mh_cycle_async(null, C.c_int(0), null, null, C.c_int(0), null, null, null) == I
    assert lib.rfsgpu_batch_fastslam_last_cycle(null, null, null, null, null, null, null, null) == I
    assert lib.rfsgpu_batch_live_counts(null, null) == I
    lib.rfsgpu_create_batch_mh.restype = C.c_int
    assert lib.rfsgpu_create_batch_mh(null, C.c_int(0), C.c_int(1), C.c_int(1), C.c_int(1), C.c_int(0), C.c_int(64)) == I


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _shut(rig):
    def f(b, c):
        c.minUpdatesBeforeResample = NEVER
        c.nParticlesMax = rig.stride
    rig.each_config(f)


def _ragged(pkg, sc):
    """4 filters x 5 particles, stride 33 (odd: waves of one workgroup belong to different filters in the 4-wave and 2-wave kernels),
    gates shut, two cycles.  -> (rig, the counts the second cycle started from)"""
    n = 5
    scens = [ref.crowded(sc, n), ref.sparse(sc, n), ref.mixed(sc, n), ref.crowded(sc, n, seed=113)]
    rig = mb.Rig(pkg, sc, scens, [4, 4, 6, 4], [50.0, 50.0, 8.0, 50.0], n, 33)
    _shut(rig)
    Zs = [scens[0]["Z"], scens[1]["Z"], scens[2]["Z"], np.zeros((0, 2))]
    rig.cycle(Zs, [0.25] * 4)
    lc, _ = rig.compare()
    c1 = rig.batch.live_counts().copy()
    print("counts after the first cycle", c1)
    assert c1[0] == 20 and c1[1] == 5 and c1[3] == 5 and 5 < c1[2] <= 30
    assert len(set(c1.tolist())) >= 3, "the second cycle must start from at least three distinct counts"
    assert np.array_equal(lc["parent"][3, :5], np.arange(5)) and np.array_equal(lc["plan"][3, :5], np.arange(5))
    # second cycle: filters 0 and 2 keep their grown sets (one hypothesis from now on), filter 1 stays, filter 3 gets its first scan
    def second(b, c):
        if b in (0, 2):
            c.maxNDataAssocHypotheses = 1
    rig.each_config(second)
    rz = np.random.default_rng(5)
    Zs = [s["Z"] + rz.normal(0, 3e-3, s["Z"].shape) for s in scens]
    rig.cycle(Zs, [0.75] * 4)
    rig.compare()
    c2 = rig.batch.live_counts()
    print("counts after the second cycle", c2)
    assert c2[0] == c1[0] and c2[1] == 5 and c2[2] == c1[2] and c2[3] == 20
    return rig, c1


@pytest.mark.gpu
def test_ragged_counts_with_the_gates_shut(pkg, sc):
    rig, _ = _ragged(pkg, sc)
    rig.close()


@pytest.mark.gpu
def test_propagation_on_ragged_counts(pkg, sc):
    """rfsgpu_batch_propagate_async after the second cycle: the live slots' poses equal the numpy reference, keyed by the slot within
    the filter."""
    rig, _ = _ragged(pkg, sc)
    B = rig.batch
    counts = B.live_counts()
    assert len(set(counts.tolist())) >= 2
    var = np.array([[1e-4, 2e-4, 1e-5], [4e-4, 1e-4, 2e-5], [0.0, 0.0, 0.0], [9e-4, 1e-4, 4e-5]])
    seeds = [77, 78, 79, 80]
    for b in range(4):
        B.set_motion_odometry(b, var[b], seeds[b])
    u = np.array([[0.10, 0.01, 0.02], [0.05, -0.02, -0.01], [0.2, 0.0, 0.03], [0.0, 0.1, 0.0]])
    before = B.get_poses().copy()
    B.propagate_async(u, 3)
    got = B.get_poses()
    for b in range(4):
        blk = B.block(b, counts[b])
        want = dl.propagate(before[blk], u[b], var[b], seeds[b], 3)        # (slot i of the filter draws with counter i)
        np.testing.assert_allclose(got[blk], want, rtol=1e-10, atol=1e-10, err_msg="filter %d" % b)
    assert np.array_equal(B.live_counts(), counts)
    rig.close()


@pytest.mark.gpu
def test_three_kinds_of_resampling_in_one_cycle(pkg, sc):
    """3 filters x 8, stride 40: filter 0 is forced (32 > nParticlesMax 24), filter 1 fires by N_eff, filter 2 runs the test and does not
    fire (the second normalisation runs)."""
    n, stride, u01 = 8, 40, [0.37, 0.61, 0.83]
    scens = [ref.crowded(sc, n), ref.crowded(sc, n, seed=114), ref.crowded(sc, n, seed=115)]
    hyps, diff = [4, 2, 2], 50.0
    rig = mb.Rig(pkg, sc, scens, hyps, [diff] * 3, n, stride)
    eff = [(2.0, 0.25), (1e9, 0.0), (1e-9, 1e-12)]
    for b in range(3):
        rig.set_resampling(b, *eff[b])
    Zs = [s["Z"] for s in scens]
    # margins, on a handle's own weights
    grown = []
    for b in range(3):
        w, g = mb.probe_weights(pkg, sc, scens[b], hyps[b], diff, stride, Zs[b])
        grown.append(g)
        assert w.size == n * hyps[b]
        near, neff = ref.resample_margins(w, u01[b], n)
        print("filter %d: grown %d, N_eff %.6g, nearest sample point / cumulative sum %.3g" % (b, w.size, neff, near))
        if b < 2:
            assert near >= 1e-9
        if b > 0:
            for t, v in ((eff[b][0], neff), (eff[b][1], neff / w.size)):
                assert t == 0.0 or abs(v / t - 1) >= 1e-6
    before = [rig.block_state(b) for b in range(3)]
    rig.cycle(Zs, u01)
    lc, occ = rig.compare()
    assert list(lc["n_after_update"]) == [32, 16, 16] and list(lc["n_after_resample"]) == [8, 8, 16]
    assert list(lc["fired"]) == [True, True, False] and list(occ) == [True, True, False]
    assert lc["n_eff"][0] == 0.0 and lc["n_eff"][1] > 0 and lc["n_eff"][2] > 0      # forced: the test did not run
    assert before[0]["n"] == 8
    # every slot of a resampled filter holds the grown-set particle its plan names (the grown set: the probe handle's, gates shut)
    for b in (0, 1):
        st = rig.block_state(b)
        plan = lc["plan"][b, :8]
        assert not np.array_equal(plan, np.arange(8))
        for i in range(8):
            s = int(plan[i])
            assert np.array_equal(st["poses"][i], grown[b]["poses"][s]) and st["sizes"][i] == grown[b]["sizes"][s]
            assert st["fov"][i] == grown[b]["fov"][s] and st["unused"][i] == grown[b]["unused"][s]
            for x, y in zip(st["maps"][i], grown[b]["maps"][s]):
                assert np.array_equal(x, y), "filter %d slot %d" % (b, i)
        assert (st["w"] == 1.0).all()
    w2 = rig.block_state(2)["w"]
    assert abs(w2.sum() - 1) < 1e-12
    rig.close()


@pytest.mark.gpu
def test_chunked_plan_and_shrink(pkg, sc):
    """2 filters x 257, stride 520, 2 hypotheses: a plan thread owns more than one particle and the shrink kernel's runs exceed one.
    Filter 0 (crowded) doubles and is forced back; filter 1 (windowed) grows by some and resamples by N_eff."""
    n, stride, u01 = 257, 520, [0.41, 0.59]
    scens = [ref.crowded(sc, n), ref.windowed(sc, n)]
    hyps, diffs = [2, 2], [50.0, 1.0]
    rig = mb.Rig(pkg, sc, scens, hyps, diffs, n, stride)

    def cfg(b, c):
        c.nParticlesMax = 513 if b == 0 else stride
    rig.each_config(cfg)
    rig.set_resampling(1, 1e9, 0.0)
    Zs = [s["Z"] for s in scens]
    for b in range(2):
        w, _ = mb.probe_weights(pkg, sc, scens[b], hyps[b], diffs[b], stride, Zs[b])
        near, neff = ref.resample_margins(w, u01[b], n)
        print("filter %d: grown %d, N_eff %.6g, nearest sample point / cumulative sum %.3g" % (b, w.size, neff, near))
        assert near >= 1e-9
        if b == 1:      # (filter 0 is forced; filter 1 decides by N_eff against 1e9 and 0)
            assert abs(neff / 1e9 - 1) >= 1e-6
    rig.cycle(Zs, u01)
    lc, _ = rig.compare()
    assert lc["n_after_update"][0] == 514 and 257 < lc["n_after_update"][1] < 514
    assert list(lc["n_after_resample"]) == [257, 257] and list(lc["fired"]) == [True, True]
    rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [16, 15])
def test_capacity_is_per_filter(pkg, sc, stride):
    """3 filters x 4, 4 hypotheses, filter 1 crowded.  Stride 16: everything fits, filter 1 ends at exactly 16.  Stride 15: filter 1
    is left as it was, filters 0 and 2 equal their handles, the next synchronising call reports filter 1 once; a further cycle with a
    sparse scene for filter 1 succeeds for all three.  (predict = 0: a static step asked for would have run before the overflow is
    known, on the handle route as well.)"""
    n = 4
    scens = [ref.sparse(sc, n), ref.crowded(sc, n), ref.sparse(sc, n, seed=202)]
    rig = mb.Rig(pkg, sc, scens, [4, 4, 4], [50.0] * 3, n, stride)
    _shut(rig)
    Zs = [s["Z"] for s in scens]
    before = rig.block_state(1)
    if stride == 16:
        rig.cycle(Zs, [0.5] * 3, predict=False)
        lc, _ = rig.compare()
        assert list(rig.batch.live_counts()) == [4, 16, 4] and not lc["overflowed"].any()
        rig.close()
        return
    rig.batch.cycle_async(False, Zs, [0.5] * 3)
    rig.batch.cycle_async(False, Zs, [0.5] * 3)        # enqueued behind the overflow: abandoned for filter 1 only
    for b in (0, 2):
        rig.handles[b].cycle_async(Zs[b], 0.5, predict=False)
        rig.handles[b].cycle_async(Zs[b], 0.5, predict=False)
    with pytest.raises(pkg.capi.EngineError) as e:
        rig.batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "filter 1" in str(e.value), str(e.value)
    rig.batch.synchronize()                             # reported once
    lc = rig.batch.last_cycle()
    assert list(lc["overflowed"]) == [False, True, False] and list(rig.batch.live_counts()) == [4, 4, 4]
    ref.assert_same_state(before, rig.block_state(1))
    for b in (0, 2):
        a, c = ref.state(rig.handles[b]), rig.block_state(b)
        ref.assert_same_state(a, c, weights=1e-12)
    # the batch goes on: a sparse scene for filter 1 (its handle takes the same state and scan)
    s1 = ref.sparse(sc, n, seed=203)
    h1 = rig.handles[1]
    x = rig.batch.get_poses()
    x[rig.batch.block(1, n)] = s1["poses"]
    rig.batch.set_poses(x, s1["pose_cov"])
    h1.set_poses(s1["poses"], s1["pose_cov"])
    P = s1["params"]
    rig.batch.configure(1, None, R=P["R"], Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"])
    h1.set_model_rngbrg(P["R"], P["Pd"], P["clutter"], P["rmax"], P["rmin"], P["rbuf"])
    for i in range(n):
        for f, slot in ((rig.batch, stride + i), (h1, i)):
            f.import_gm(slot, np.zeros(s1["w"][i].shape), s1["mean"][i], s1["cov"][i])
    Zs[1] = s1["Z"]
    rig.cycle(Zs, [0.5] * 3, predict=False)
    lc, _ = rig.compare()
    assert not lc["overflowed"].any() and rig.batch.live_counts()[1] == 4
    rig.close()


@pytest.mark.gpu
def test_mixed_prune_thresholds_and_kinds(pkg, sc):
    """Filter 1 has fewer measurements than its pruningMeasurementsThreshold while the others prune; filter 2 keeps one hypothesis
    among multi-hypothesis filters."""
    n = 6
    scens = [ref.crowded(sc, n), ref.crowded(sc, n, seed=116), ref.mixed(sc, n)]
    rig = mb.Rig(pkg, sc, scens, [3, 3, 1], [50.0, 50.0, 8.0], n, 19)
    _shut(rig)

    def cfg(b, c):
        c.pruningMeasurementsThreshold = 9 if b == 1 else 0
        c.mapExistencePruneThreshold = -0.5        # (so that a prune removes something: missed landmarks fall below it)
    rig.each_config(cfg)
    Zs = [s["Z"] for s in scens]
    assert len(Zs[1]) == 8
    sizes0 = np.asarray(rig.batch.gm_sizes()).copy()
    rig.cycle(Zs, [0.3] * 3)
    lc, _ = rig.compare()
    assert list(lc["n_after_update"]) == [18, 18, 6]
    sizes = np.asarray(rig.batch.gm_sizes())
    pruned = [bool((sizes[rig.batch.block(b, lc["n_after_update"][b])] < sizes0[b * 19]).any()) for b in range(3)]
    print("some particle of the filter lost a landmark to the prune:", pruned)
    assert pruned[0] and not pruned[1]
    rig.close()


@pytest.mark.gpu
def test_batch_of_one_equals_a_plain_handle(pkg, sc):
    """Gates shut, two cycles: the first multiplies the particles (2, 4 or 6 hypotheses each), the second runs on the grown set."""
    n = 7
    rig = mb.Rig(pkg, sc, [ref.mixed(sc, n)], [6], [8.0], n, 42)
    _shut(rig)
    rz = np.random.default_rng(9)
    Z = rig.scens[0]["Z"]
    rig.cycle([Z], [0.2])
    lc, _ = rig.compare()
    grown = int(lc["n_after_update"][0])
    assert n < grown <= 42 and len(set(np.bincount(lc["parent"][0, :grown], minlength=n).tolist())) >= 2
    rig.each_config(lambda b, c: setattr(c, "maxNDataAssocHypotheses", 1))
    rig.cycle([Z + rz.normal(0, 3e-3, Z.shape)], [0.6])
    lc, _ = rig.compare()
    assert lc["n_after_update"][0] == grown == rig.batch.live_counts()[0]
    rig.close()


@pytest.mark.gpu
def test_five_cycles_enqueued_back_to_back(pkg, sc):
    """No call between the five cycles reads or waits; the same five with last_cycle after each end in the same state."""
    n, hyp = 8, 2
    scens = [ref.crowded(sc, n), ref.crowded(sc, n, seed=117)]
    rz = np.random.default_rng(4)
    Zs = [[s["Z"] + rz.normal(0, 3e-3, s["Z"].shape) for s in scens] for _ in range(5)]
    Zs[3][0] = np.zeros((0, 2))                                   # an empty scan in the middle for filter 0
    draws = [[0.11, 0.21], [0.52, 0.62], [0.93, 0.03], [0.34, 0.44], [0.75, 0.85]]
    rigs = []
    decided = planned = 0
    for sync in (False, True):
        rig = mb.Rig(pkg, sc, scens, [hyp, hyp], [50.0, 50.0], n, 32)     # nParticlesMax 24: 8 -> 16 stays, 16 -> 32 is forced back to 8
        rig.each_config(lambda b, c: setattr(c, "minUpdatesBeforeResample", 2))
        for Z, u in zip(Zs, draws):
            snap = rig.snapshot() if sync else None
            rig.cycle(Z, u)
            if sync:
                rig.batch.last_cycle()
                # the margins of this cycle's decisions and plans, on the handles (the same in both rigs)
                nd, npl = rig.assert_margins(snap, Z, u, lambda b, p: sc.apply_params(p, scens[b]["params"]))
                decided += nd
                planned += npl
        rigs.append(rig)
    print("N_eff decisions with their margins asserted: %d, plans: %d" % (decided, planned))
    assert planned >= 1
    a, b = rigs
    la, _ = a.compare()
    lb, _ = b.compare()
    for k in la:
        assert np.array_equal(la[k], lb[k]), k
    for f in range(2):
        ref.assert_same_state(a.block_state(f), b.block_state(f))
    a.close(); b.close()


def _sim_config():
    import xml.etree.ElementTree as ET
    t = ET.parse(os.path.join(ROOT, "tests", "golden", "mhfastslam2dSim_c1.xml")).getroot()
    return dict(max_hypotheses=int(t.find("filter/update/maxNDataAssocHypotheses").text),
                max_loglik_diff=float(t.find("filter/update/maxDataAssocLogLikelihoodDiff").text),
                min_log_likelihood=float(t.find("filter/weighting/minLogMeasurementLikelihood").text),
                existence_prune_thr=float(t.find("filter/prune/threshold").text),
                eff_n=float(t.find("filter/resampling/effNParticle").text), min_updates=int(t.find("filter/resampling/minTimesteps").text))


@pytest.mark.gpu
def test_thirty_simulator_steps_against_three_handles(pkg, sc):
    """3 filters x 16, the values of tests/golden/mhfastslam2dSim_c1.xml (3 hypotheses, window 3.0), 30 simulator steps with the poses at
    the ground truth: counts and decisions every step, everything every 5th."""
    drv = pkg.sim2d_driver
    P = dict(drv.C1_FASTSLAM_SIM, **_sim_config(), kmax=120)
    assert P["max_hypotheses"] == 3 and P["max_loglik_diff"] == 3.0
    # (stride: nParticlesMax x hypotheses.  A set at nParticlesMax = 48 is not forced back, and with minTimesteps 2 the next update can
    #  multiply it again before any resampling: 48 slots overflow at step 2, on a handle with max_particles 48 just as well)
    nF, n, stride = 3, 16, 144
    Ps = [dict(P, Pd=pd) for pd in (0.99, 0.9, 0.7)]
    datas = [drv.generate(Pb, traj_seed=3 + b, kmax=31) for b, Pb in enumerate(Ps)]
    datas[1]["Z"][7] = np.zeros((0, 2))          # two dropped scans (the generator gives none within 30 steps): one filter's update is
    datas[2]["Z"][12] = np.zeros((0, 2))         # only counted while the others' run
    draws = np.random.default_rng(8).random((31, nF))
    batch = pkg.MHFastSLAMBatch(nF, n, stride, gm_capacity=64)
    hs = [mb.handle(pkg, n, stride) for _ in range(nF)]
    for b, (h, Pb) in enumerate(zip(hs, Ps)):
        drv.configure(h, Pb)
        h.config = h.get_filter_config()
        h.fs_config = drv.fastslam_config(h, Pb)
        h.fs_config.nParticlesMax = 3 * n
        h.setEffectiveParticleCountThreshold(Pb["eff_n"])
        c = drv.configure_fastslam_batch_filter(batch, b, Pb)
        c.nParticlesMax = 3 * n
        batch.configure_fastslam(b, c)
        batch.set_resampling(b, h.effNParticles_t, h.effNParticles_t_percent)
    rig = mb.Rig.of(pkg, sc, batch, hs, n, stride)
    fired = empty = grew = decided = planned = 0
    for k in range(1, 31):
        Zs = [d["Z"][k] for d in datas]
        empty += sum(len(Z) == 0 for Z in Zs)
        x = np.concatenate([np.tile(d["gt"][k], (stride, 1)) for d in datas])
        batch.cycle_async(True, Zs, draws[k], poses=x, pose_cov=np.zeros((3, 3)))
        for b, h in enumerate(hs):
            h.set_poses(np.tile(datas[b]["gt"][k], (h.n, 1)), np.zeros((3, 3)))
        snap = rig.snapshot()
        for b, h in enumerate(hs):
            h.cycle_async(Zs[b], float(draws[k, b]), predict=True)
        nd, npl = rig.assert_margins(snap, Zs, draws[k], lambda b, p: drv.configure(p, Ps[b]))      # before anything is compared
        decided += nd
        planned += npl
        lc, _ = rig.compare(maps=(k % 5 == 0 or k == 30))
        fired += int(lc["fired"].sum())
        grew += int((lc["n_after_update"] > n).sum())
    print("resamplings %d (plans with margins asserted %d, N_eff decisions %d), empty scans %d, updates that multiplied particles %d" % (fired, planned, decided, empty, grew))
    assert fired >= 1 and empty >= 1 and grew >= 1 and planned == fired and decided >= 1
    rig.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_untouched(pkg, sc):
    U, I = pkg.capi.ERR_UNSUPPORTED, pkg.capi.ERR_INVALID
    # creation
    for n_per, stride, code in ((4, 2049, U), (8, 7, I)):
        with pytest.raises(pkg.capi.EngineError) as e:
            pkg.MHFastSLAMBatch(2, n_per, stride, gm_capacity=64)
        assert e.value.status == code
    n, stride = 4, 12
    scens = [ref.crowded(sc, n), ref.sparse(sc, n)]
    rig = mb.Rig(pkg, sc, scens, [2, 2], [50.0, 50.0], n, stride)
    _shut(rig)
    B = rig.batch
    Zs = [s["Z"] for s in scens]
    rig.cycle(Zs, [0.5, 0.5])
    rig.compare()

    def snapshot():
        return [rig.block_state(b) for b in range(2)], B.live_counts().copy(), [np.array(a) for a in B.get_particle_ids()]

    def same(a, b):
        for x, y in zip(a[0], b[0]):
            ref.assert_same_state(x, y)
        assert np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    before = snapshot()
    N = B.n
    assert N == 2 * stride
    nz = np.array([2, 2], dtype=np.int32)
    calls = {
        "rfsgpu_batch_cycle_async": lambda: B.batch_cycle_async(True, Zs),
        "rfsgpu_batch_fastslam_cycle_async": lambda: B.batch_fastslam_cycle_async(True, Zs),
        "rfsgpu_batch_resample_async": lambda: B.resample_async(nz, 1),
        "rfsgpu_batch_resample_apply": lambda: B.batch_resample_apply(np.arange(N), np.ones(2)),
        "rfsgpu_batch_last_resample": lambda: B.last_resample(),
        "rfsgpu_batch_resample_counts": lambda: B.resample_counts(),
        "rfsgpu_batch_weight_sums": lambda: B.batch_weight_sums(),
        "set_ground_truth": lambda: B.set_ground_truth(np.zeros((3, 2))),
        "error_log_create": lambda: B.error_log_create(4),
        "step_error_async": lambda: B.step_error_async(np.zeros(2), np.zeros((2, 3))),
        "step_error": lambda: B.step_error(np.zeros(2), np.zeros((2, 3))),
        "get_map_estimate": lambda: B.get_map_estimate(),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.capi.EngineError) as e:
            call()
        assert e.value.status == U and "multi-hypothesis" in str(e.value), (name, str(e.value))
        same(before, snapshot())
    # configuration
    for field, value, word in (("maxNDataAssocHypotheses", 17, "[1, 16]"), ("maxNDataAssocHypotheses", 0, "[1, 16]"),
                               ("landmarkCandidateMeasurementCountThreshold", 2, "landmarkCandidateMeasurementCountThreshold")):
        c = mb.copy_struct(rig.handles[0].fs_config)
        setattr(c, field, value)
        with pytest.raises(pkg.capi.EngineError) as e:
            B.batch_set_fastslam_config(1, c)
        assert e.value.status == U and word in str(e.value) and "filter 1" in str(e.value), str(e.value)
    # a draw of 1.0 names its filter
    with pytest.raises(pkg.capi.EngineError) as e:
        B.cycle_async(True, Zs, [0.5, 1.0])
    assert e.value.status == I and "filter 1" in str(e.value) and "u01" in str(e.value)
    same(before, snapshot())
    # ... and an ordinary batch still refuses two hypotheses and does not know the new cycle
    plain = pkg.FastSLAMBatch(2, 4, gm_capacity=64)
    c = plain.default_fastslam_config()
    c.maxNDataAssocHypotheses = 2
    with pytest.raises(pkg.capi.EngineError) as e:
        plain.batch_set_fastslam_config(0, c)
    assert e.value.status == U
    plain.close()
    # the batch goes on after all that
    rig.each_config(lambda b, c: setattr(c, "maxNDataAssocHypotheses", 1))
    rig.cycle(Zs, [0.5, 0.5])
    rig.compare()
    rig.close()
