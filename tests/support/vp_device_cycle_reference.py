"""Helpers of tests/test_fastslam_vp_device_cycle.py: the pose bookkeeping a host keeps under particle copies and resampling plans,
pairs of FastSLAM objects (the host-stop route and the device cycle) on either model with landmark candidate lists, the state
that is compared between them, and the pattern planted beyond the live particle count."""
import numpy as np

from tests.support import mh_device_cycle_reference as mh

NEVER = 1000          # minUpdatesBeforeResample that no test reaches


def follow_poses(x, parents, plan=None):
    """Host poses after an update whose copies came from `parents` (slot -> source slot, over the grown set) and, where a resampling
    fired, its `plan` (slot -> slot of the grown set): x[parents] then x[plan], as vp_driver.VictoriaParkRun keeps them."""
    x = np.asarray(x)[np.asarray(parents, dtype=np.int64)]
    return x if plan is None else x[np.asarray(plan, dtype=np.int64)]


def follow_poses_loop(x, parents, plan=None):
    """The same, one slot at a time."""
    grown = [list(x[int(p)]) for p in parents]
    if plan is None:
        return np.array(grown, dtype=np.float64).reshape(len(grown), -1)
    return np.array([grown[int(s)] for s in plan], dtype=np.float64).reshape(len(plan), -1)


def candidate_config(cfg, thr, cur_thr):
    cfg.landmarkCandidateMeasurementCountThreshold = thr
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = cur_thr
    cfg.landmarkCandidateMeasurementCheckThreshold = 3
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.mapExistencePruneThreshold = -5.0
    return cfg


def make_pair(pkg, sc, scen, hyp, thr, cur_thr, cap, diff=50.0, gm_capacity=192):
    """(host-stop route, device cycle): two FastSLAM objects of the scenario's model with the same state, zero log-odds maps (as
    tests/test_mh_fastslam_device_cycle.py loads them), candidate lists configured, `cap` particle slots."""
    model = pkg.capi.MODEL_VICTORIAPARK_3D if scen.get("model") == "vp" else pkg.capi.MODEL_RNGBRG_2D
    out = []
    for dc in (False, True):
        f = pkg.FastSLAM(scen["n"], gm_capacity=gm_capacity, max_hypotheses=max(hyp, 2), device_cycle=dc, max_particles=cap, model=model)
        sc.load_scenario(f, scen)
        for i in range(scen["n"]):
            f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
        f.config = f.get_filter_config()
        candidate_config(f.fs_config, thr, cur_thr)
        f.fs_config.maxNDataAssocHypotheses = hyp
        f.fs_config.maxDataAssocLogLikelihoodDiff = diff
        f.fs_config.nParticlesMax = cap
        f.fs_config.minUpdatesBeforeResample = NEVER
        f.set_fastslam_config(f.fs_config)
        out.append(f)
    return out


def warm_up(fs, Z):
    """One single-hypothesis update through rfsgpu_fastslam_update on every handle (the same kernels on the same inputs: the same
    bits), so that the update under test starts from maps with history and non-empty candidate lists."""
    for f in fs:
        cfg = f.get_fastslam_config()
        keep = cfg.maxNDataAssocHypotheses
        cfg.maxNDataAssocHypotheses = 1
        f.set_fastslam_config(cfg)
        f.predict_map()
        f.fastslam_update(Z)
        f.normalize_weights(f.weight_sums()[0])
        cfg.maxNDataAssocHypotheses = keep
        f.set_fastslam_config(cfg)


def state(f):
    """mh.state plus the landmark candidate lists (means, covariances, support and check counts) and the particle ids."""
    s = mh.state(f)
    s["cands"] = [tuple(np.array(x) for x in f.export_birth_candidates(i)) for i in range(s["n"])]
    s["ids"] = tuple(np.array(x) for x in f.get_particle_ids())
    return s


def assert_same_state(a, b):
    mh.assert_same_state(a, b)
    for i, (ca, cb) in enumerate(zip(a["cands"], b["cands"])):
        for x, y, what in zip(ca, cb, ("mean", "cov", "support", "check")):
            assert x.shape == y.shape and np.array_equal(x, y), "candidate %s of particle %d" % (what, i)
    for x, y in zip(a["ids"], b["ids"]):
        assert np.array_equal(x, y), "particle ids"


POISON_W, POISON_COUNT, POISON_CAND = -7.25, 3, 2


def poison(f, first):
    """Plant a pattern in every slot from `first` to max_particles: weight, mixture size, candidate count, first Gaussian."""
    npl = 7 if f.dm == 2 else 11
    for s in range(first, f.max_particles):
        f.debug_slot(s, (POISON_W - s, POISON_COUNT, POISON_CAND, 0.5 + s + np.arange(npl)))


def assert_poison(f, first):
    npl = 7 if f.dm == 2 else 11
    assert first < f.max_particles
    for s in range(first, f.max_particles):
        w, c, k, g = f.debug_slot(s)
        assert (w, c, k) == (POISON_W - s, POISON_COUNT, POISON_CAND), "slot %d beyond the live count was written: %r" % (s, (w, c, k))
        assert np.array_equal(g, 0.5 + s + np.arange(npl)), "first Gaussian of slot %d beyond the live count was written" % s
